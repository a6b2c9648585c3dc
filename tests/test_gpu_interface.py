"""GPU parity of the MD front ends: the LAMMPS / GROMACS models and the ASE calculator against the
CPU oracle evaluated in the model's own units and converted with the golden unit factors.  Run:  pytest tests -m gpu"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from xequinet_amd.data import synthetic as syn

from . import test_gpu_parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNITS = json.load(open(os.path.join(P.G, "units.json")))
FACTOR = {(a, b): v for a, b, v in UNITS["pairs"]}


@pytest.fixture(autouse=True)
def _model_units():
    from xequinet_amd.utils import units as U

    saved = dict(U.DEFAULT_UNITS_MAP)
    U.set_default_units({"energy": "eV"})   # what a checkpoint's config carries (default_units)
    yield
    U.DEFAULT_UNITS_MAP.clear()
    U.DEFAULT_UNITS_MAP.update(saved)


def _twin(cls, dtype, **kw):
    """an MD model with the weights of P._build's model + the oracle over those weights"""
    base, oracle = P._build(dtype)
    m = cls(**kw).eval().requires_grad_(False).to(dtype).to(DEV)
    m.load_state_dict(base.state_dict())
    return m, oracle


def _oracle_in(pos, z, ptr, ei, extra=None):
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    d = {"pos": torch.tensor(pos, dtype=torch.float64), "atomic_numbers": torch.tensor(z.astype(np.int64)),
         "edge_index": torch.tensor(ei), "batch": torch.tensor(batch), "ptr": torch.tensor(ptr)}
    for k, v in (extra or {}).items():
        d[k] = torch.tensor(v, dtype=torch.float64)
    return d


@pytest.mark.parametrize("style,e_pair,f_pair,len_pair", [
    ("metal", None, None, None),
    ("real", ("eV", "kcal/mol"), ("eV/Angstrom", "kcal/mol/Angstrom"), None),
    ("electron", ("Hartree", "eV"), ("Hartree/Bohr", "eV/Angstrom"), ("Bohr", "Angstrom")),
])
@pytest.mark.parametrize("replay", [False, True])
def test_lammps_model_units_and_values(style, e_pair, f_pair, len_pair, replay):
    from xequinet_amd.interface import XPaiNNLMP, resolve_jit_model

    dtype = torch.float64
    model, oracle = _twin(XPaiNNLMP, dtype, unit_style=style, replay=replay, tune_gemms=False)
    assert type(resolve_jit_model("lmp", unit_style=style)) is XPaiNNLMP
    pos, z, ptr = syn.synth_aspirin()
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 5.0)
    want = oracle(_oracle_in(pos, z, ptr, ei), compute_forces=True)
    e_fac = 1.0 if e_pair is None else (FACTOR[e_pair] if style == "real" else 1.0 / FACTOR[e_pair])
    f_fac = 1.0 if f_pair is None else (FACTOR[f_pair] if style == "real" else 1.0 / FACTOR[f_pair])
    l_fac = 1.0 if len_pair is None else FACTOR[len_pair]        # engine length -> Angstrom
    np.testing.assert_allclose(model.cutoff_radius, 5.0 / l_fac, rtol=1e-12)
    pos_engine = pos / l_fac
    data = {"pos": P._t(pos_engine, dtype), "atomic_numbers": P._t(z.astype(np.int32)), "edge_index": P._t(ei)}
    keep = data["pos"].clone()
    for _ in range(2):   # the second call replays the captured graph
        with torch.enable_grad():
            got = model(dict(data), compute_forces=True, compute_virial=False)
        np.testing.assert_allclose(got["energy"].detach().cpu().numpy(), want["energy"].numpy() * e_fac, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(got["forces"].detach().cpu().numpy(), want["forces"].numpy() * f_fac, rtol=0,
                                   atol=1e-8 * max(1.0, np.abs(want["forces"].numpy()).max() * f_fac))
    assert torch.equal(data["pos"], keep), "the caller's positions are not rescaled in place"
    assert got["atomic_energies"].shape == (21,)


def test_lammps_model_periodic_virial_and_replay_is_bitwise():
    from xequinet_amd.interface import XPaiNNLMP

    dtype = torch.float32
    f = P._load("radius_graph_pbc_water192.npz")
    _, z, ptr, _ = syn.synth_water_box(4, seed=5)
    eager, oracle = _twin(XPaiNNLMP, dtype, unit_style="real")
    fast, _ = _twin(XPaiNNLMP, dtype, unit_style="real", replay=True, tune_gemms=False)
    extra = {"cell": f["cell"].astype(np.float64), "cell_offsets": f["cell_offsets"].astype(np.float64)}
    want = oracle(_oracle_in(f["pos"].astype(np.float64), z, ptr, f["edge_index"], extra), compute_forces=True, compute_virial=True)
    mk = lambda: {"pos": P._t(f["pos"], dtype), "atomic_numbers": P._t(z.astype(np.int32)), "edge_index": P._t(f["edge_index"]),
                  "cell": P._t(f["cell"], dtype), "cell_offsets": P._t(f["cell_offsets"], dtype),
                  "pbc": torch.tensor([[True, True, True]], device=DEV)}
    with torch.enable_grad():
        a = eager(mk(), compute_forces=True, compute_virial=True)
        b = fast(mk(), compute_forces=True, compute_virial=True)
        c = fast(mk(), compute_forces=True, compute_virial=True)
    kc = FACTOR[("eV", "kcal/mol")]
    V, Vref = a["virial"].detach().cpu().double().numpy(), want["virial"].numpy() * kc
    assert V.shape == (1, 3, 3)
    np.testing.assert_allclose(V, Vref, rtol=0, atol=2e-3 * np.abs(Vref).max())        # fp32, ~50 neighbours/atom (see test_gpu_parity)
    np.testing.assert_allclose(a["forces"].detach().cpu().double().numpy(), want["forces"].numpy() * FACTOR[("eV/Angstrom", "kcal/mol/Angstrom")],
                               rtol=0, atol=2e-3 * np.abs(want["forces"].numpy()).max() * kc)
    for k in ("energy", "forces", "virial", "atomic_energies"):
        assert torch.equal(a[k].detach(), b[k].detach()) and torch.equal(b[k].detach(), c[k].detach()), k


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("periodic", [False, True])
def test_gromacs_model_energy_and_autograd_forces(periodic, replay):
    from xequinet_amd.interface import XPaiNNGMX

    dtype = torch.float64
    model, oracle = _twin(XPaiNNGMX, dtype, replay=replay, tune_gemms=False)
    nm = FACTOR[("nm", "Angstrom")]
    if periodic:
        f = P._load("single_radius_graph_water192.npz")
        a = P._load("radius_graph_pbc_water192.npz")
        _, z, ptr, _ = syn.synth_water_box(4, seed=5)
        pos, cell = a["pos"].astype(np.float64), a["cell"][0].astype(np.float64)
        ei, co = f["edge_index"], f["cell_offsets"].astype(np.float64)
        extra = {"cell": cell[None], "cell_offsets": co}
        box, pbc = P._t(cell / nm, dtype), torch.tensor([True, True, True], device=DEV)
    else:
        pos, z, ptr = syn.synth_aspirin()
        ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 5.0)
        extra, box, pbc = None, None, None
    want = oracle(_oracle_in(pos, z, ptr, ei, extra), compute_forces=True)
    kj = FACTOR[("eV", "kcal/mol")] * 4.184
    fref = want["forces"].numpy() * FACTOR[("eV/Angstrom", "kJ/(mol*nm)")]
    for _ in range(2):   # with replay: capture, then one graph launch
        x = P._t(pos / nm, dtype).requires_grad_(True)
        energy = model(x, P._t(z.astype(np.int64)), box, pbc)
        (g,) = torch.autograd.grad(energy.sum(), x)
        np.testing.assert_allclose(energy.detach().cpu().numpy(), want["energy"].numpy() * kj, rtol=1e-9)
        np.testing.assert_allclose(-g.cpu().numpy(), fref, rtol=0, atol=1e-8 * np.abs(fref).max())
    np.testing.assert_allclose(model.forces_unit_factor, FACTOR[("eV/Angstrom", "kJ/(mol*nm)")], rtol=1e-12)


class _Atoms:
    """the slice of ase.Atoms the calculator reads"""

    def __init__(self, pos, z, cell=None, pbc=(False, False, False)):
        self.pos, self.z = np.array(pos, dtype=np.float64), np.array(z)
        self.cell = np.zeros((3, 3)) if cell is None else np.array(cell, dtype=np.float64)
        self.pbc = np.array(pbc, dtype=bool)

    def copy(self):
        return _Atoms(self.pos, self.z, self.cell, self.pbc)

    def get_pbc(self):
        return self.pbc

    def get_cell(self):
        return self.cell

    def get_atomic_numbers(self):
        return self.z

    def get_volume(self):
        return abs(np.linalg.det(self.cell))

    def get_positions(self, wrap=False):
        if not wrap or not self.pbc.any():
            return self.pos.copy()
        frac = np.linalg.solve(self.cell.T, self.pos.T).T
        frac[:, self.pbc] %= 1.0
        return frac @ self.cell

    def wrap(self):
        self.pos = self.get_positions(wrap=True)


@pytest.mark.parametrize("replay", [False, True])
def test_ase_calculator_molecule_and_periodic_box(replay):
    from xequinet_amd.interface import XequiCalculator
    from xequinet_amd.interface.ase_calculator import _HAVE_ASE

    if _HAVE_ASE:
        pytest.skip("duck-typed Atoms stand-in is for images without ASE")
    dtype = torch.float64
    model, oracle = P._build(dtype)
    calc = XequiCalculator(model=model, dtype="float64", replay=replay, tune_gemms=False)
    # molecule: energy / energies / forces
    pos, z, ptr = syn.synth_aspirin()
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 5.0)
    want = oracle(_oracle_in(pos, z, ptr, ei), compute_forces=True)
    for _ in range(2):
        calc.calculate(_Atoms(pos, z), ["energy", "forces"])
        np.testing.assert_allclose(calc.results["energy"], want["energy"].item(), rtol=1e-9)
        np.testing.assert_allclose(calc.results["forces"], want["forces"].numpy(), rtol=0, atol=1e-8)
        np.testing.assert_allclose(calc.results["energies"], want["atomic_energies"].numpy(), rtol=1e-9, atol=1e-10)
    assert "stress" not in calc.results
    # periodic water box, atoms shifted out of the cell: wrapped by the calculator; stress from the virial
    f = P._load("radius_graph_pbc_water192.npz")
    _, zw, ptrw, _ = syn.synth_water_box(4, seed=5)
    posw, cell = f["pos"].astype(np.float64), f["cell"][0].astype(np.float64)
    ei_w, co_w = f["edge_index"], f["cell_offsets"].astype(np.float64)
    wantw = oracle(_oracle_in(posw, zw, ptrw, ei_w, {"cell": cell[None], "cell_offsets": co_w}), compute_forces=True, compute_virial=True)
    shifted = posw + np.array([2, -1, 1]) @ cell
    calc.calculate(_Atoms(shifted, zw, cell, (True, True, True)))
    np.testing.assert_allclose(calc.results["energy"], wantw["energy"].item(), rtol=1e-9)
    np.testing.assert_allclose(calc.results["forces"], wantw["forces"].numpy(), rtol=0, atol=1e-8)
    v = wantw["virial"].numpy()[0]
    voigt = np.array([v[0, 0], v[1, 1], v[2, 2], v[1, 2], v[0, 2], v[0, 1]]) / abs(np.linalg.det(cell))
    np.testing.assert_allclose(calc.results["stress"], voigt, rtol=0, atol=1e-9 * max(1.0, np.abs(voigt).max()))


def test_ase_calculator_from_checkpoint_file(tmp_path):
    """The reference's construction path (ase_calculator.py:46-73): `ckpt_file` holding `config` (model name, kwargs,
    default units) and `model` (state dict, here with e3nn's weight-less bookkeeping entries a real checkpoint carries)."""
    from xequinet_amd.interface import XequiCalculator
    from xequinet_amd.interface.ase_calculator import _HAVE_ASE

    if _HAVE_ASE:
        pytest.skip("duck-typed Atoms stand-in is for images without ASE")
    kw = dict(node_dim=32, node_irreps="32x0e+16x1o+8x2e", num_basis=8, cutoff=4.0, action_blocks=2, hidden_dim=16)
    model, oracle = P._build(torch.float32, **kw)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    sd["mods.message_0.rsh_conv.weight"] = torch.empty(0)                       # e3nn-only entries are dropped on load
    sd["mods.update_0.invariant.tp.output_mask"] = torch.ones(56)
    path = tmp_path / "model.pt"
    torch.save({"config": {"model_name": "xpainn", "model_kwargs": kw, "default_units": {"energy": "kcal/mol"}}, "model": sd}, path)
    calc = XequiCalculator(ckpt_file=str(path), device="cuda")
    pos, z, ptr = syn.synth_aspirin()
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 4.0)
    want = oracle(_oracle_in(pos, z, ptr, ei), compute_forces=True)
    calc.calculate(_Atoms(pos, z), ["energy", "forces"])
    kcal = 1.0 / FACTOR[("eV", "kcal/mol")]                                      # model units (kcal/mol) -> eV
    np.testing.assert_allclose(calc.results["energy"], want["energy"].item() * kcal, rtol=1e-5, atol=1e-4 * kcal)
    np.testing.assert_allclose(calc.results["forces"], want["forces"].numpy() * kcal, rtol=0, atol=1e-4 * kcal)
    assert calc.model.cutoff_radius == 4.0 and next(calc.model.parameters()).is_cuda


def test_replay_with_timed_gemm_selection_meets_the_fp32_parity_bar():
    """GraphedModel(tune_gemms=True), the MD default: library GEMM kernels are timed per shape in the warm-up runs and
    the captured graph uses the picks.  Which fp32 kernel wins varies from run to run, so the check is the parity bar
    of the eager path itself (test_gpu_parity._check_model: fp64 oracle, fp32 tolerance) for the capture and the
    replay.  The switch (PyTorch TunableOp) is process-wide and is turned off again afterwards."""
    from xequinet_amd.interface import XPaiNNLMP

    dtype = torch.float32
    f = P._load("radius_graph_pbc_water192.npz")
    _, z, ptr, _ = syn.synth_water_box(4, seed=5)
    fast, oracle = _twin(XPaiNNLMP, dtype, unit_style="metal", replay=True, tune_gemms=True)
    extra = {"cell": f["cell"].astype(np.float64), "cell_offsets": f["cell_offsets"].astype(np.float64)}
    try:
        b, _ = P._check_model(fast, oracle, f["pos"].astype(np.float64), z, ptr, f["edge_index"], dtype, extra=extra)
        c, _ = P._check_model(fast, oracle, f["pos"].astype(np.float64), z, ptr, f["edge_index"], dtype, extra=extra)
    finally:
        torch.cuda.tunable.enable(False)
    assert fast._replay.captures == 1
    assert torch.equal(b["forces"], c["forces"]) and torch.equal(b["energy"], c["energy"])


# ------------------------------------------------------------------ TorchScript front ends (registered xeq:: operators)
def _native_vs_python(dtype, periodic, n_mol=24, trace=False, own_list=False):
    """xeq::xpainn_eval (C++: csrc/xeq_torch.cpp) against the Python modules (nn/fused.py): same kernels, same order.
    ``trace``: additionally the two fronts' launch sequences (entry-point names, include/xeq.h: xeq_launch_names) of one evaluation each,
    both building the sorted views and walk plans themselves (a fresh EdgeGraph with the list builder's promises for the Python front)."""
    from xequinet_amd import keys, lib, ops
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.interface.scripted import XPaiNNNative

    model, _ = P._build(dtype)
    native = XPaiNNNative(model)
    if periodic:
        f = P._load("radius_graph_pbc_water192.npz")
        _, z, ptr, _ = syn.synth_water_box(4, seed=5)
        data = {"pos": P._t(f["pos"], dtype), "atomic_numbers": P._t(z.astype(np.int32)), "edge_index": P._t(f["edge_index"]),
                "ptr": P._t(ptr), "batch": P._t(np.zeros(len(z), dtype=np.int64)), "cell": P._t(f["cell"], dtype),
                "cell_offsets": P._t(f["cell_offsets"], dtype)}
        cs, sym = True, False
        if own_list:   # the list of this package's own periodic search: the same edges, with the builder's promise (every edge with its mirror)
            b = NeighborTransform(5.0)(XequiBatch(data["pos"], data["atomic_numbers"], data["ptr"], pbc=P._t(np.array([[True, True, True]])),
                                                  cell=data["cell"]))
            assert torch.equal(b.edge_index, data["edge_index"]) and torch.equal(b.cell_offsets, data["cell_offsets"])
            data, sym = b.to_dict(), True
            assert data[keys.EDGE_GRAPH].mirror_walk
    else:
        pos, z, ptr = syn.synth_qm9_batch(n_mol, seed=13)
        b = NeighborTransform(5.0)(XequiBatch(P._t(pos, dtype), P._t(z), P._t(ptr)))
        data = b.to_dict()
        cs, sym = True, True

    def py():
        d = dict(data)
        if trace:
            d[keys.EDGE_GRAPH] = ops.EdgeGraph(data["edge_index"], data["pos"].shape[0], center_sorted=cs, ptr=data["ptr"], symmetric=sym,
                                               cell_offsets=data.get("cell_offsets") if sym else None)
        with torch.enable_grad():
            return model(d, compute_forces=True, compute_virial=periodic)

    def cc():
        return native(data["pos"].detach(), data["atomic_numbers"], data["edge_index"], data["ptr"], data.get("cell"),
                      data.get("cell_offsets"), cs, sym, True, periodic)

    if not trace:
        want = py()
        return cc(), want
    py(), cc()                                               # packed weights, element tables, cached constants: not part of a steady evaluation
    c0 = lib.launch_count()
    want = py()
    seq_py = lib.launch_names(c0)
    c0 = lib.launch_count()
    got = cc()
    return got, want, seq_py, lib.launch_names(c0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("periodic", [False, True])
def test_native_operator_equals_python_modules_bitwise(dtype, periodic):
    got, want = _native_vs_python(dtype, periodic)
    assert torch.equal(got[0], want["energy"].detach()), (got[0] - want["energy"]).abs().max()
    assert torch.equal(got[1], want["atomic_energies"].detach())
    assert torch.equal(got[2], want["forces"].detach()), (got[2] - want["forces"]).abs().max()
    if periodic:
        assert torch.equal(got[3], want["virial"].detach()), (got[3] - want["virial"]).abs().max()


def test_both_fronts_on_this_package_s_periodic_list():
    """A periodic box whose list comes from this package's own search: both fronts take the mirror map (xeq_reverse_edge_map_pbc: no sort
    by neighbor, the reverse pass walks the forward plan) -- the same launches in the same order, results bit for bit, no sort launch."""
    got, want, seq_py, seq_cc = _native_vs_python(torch.float32, True, trace=True, own_list=True)
    assert seq_py == seq_cc, "\n".join(f"{a:36s} {b}" for a, b in zip(seq_py + ["-"] * len(seq_cc), seq_cc + ["-"] * len(seq_py)) if a != b)
    assert "xeq_reverse_edge_map_pbc" in seq_py and not any(n.startswith("xeq_csr_by_key") for n in seq_py)
    assert sum(n.startswith("xeq_message_wq_plan") for n in seq_py) == 4          # ONE walk plan (four launches), not two
    assert torch.equal(got[0], want["energy"].detach()) and torch.equal(got[2], want["forces"].detach())
    assert torch.equal(got[3], want["virial"].detach())


@pytest.mark.parametrize("n_mol", [24, 400])
def test_both_fronts_issue_the_same_launch_sequence(n_mol):
    """One kernel sequence, two fronts: the entry points of libxeq_hip.so that one f32 open-boundary force evaluation launches -- through the
    Python modules and through xeq::xpainn_eval -- are the same names in the same order (24 molecules: the chain of small node kernels;
    400 molecules, 7 187 atoms: the fused node blocks), and the results are bit for bit equal at both sizes.  The second holds because
    both fronts seed the reverse pass with MINUS one: the node block's bf16 matrix products are not symmetric in the sign
    (profiles/r05_mfma_sign.txt), a +1 seed negated afterwards differs in the last bits."""
    got, want, seq_py, seq_cc = _native_vs_python(torch.float32, False, n_mol=n_mol, trace=True)
    assert seq_py == seq_cc, "\n".join(f"{a:36s} {b}" for a, b in zip(seq_py + ["-"] * len(seq_cc), seq_cc + ["-"] * len(seq_py)) if a != b)
    assert ("xeq_node_block_fwd" in seq_py) == (n_mol >= 400) and "xeq_first_block_front" in seq_py and "xeq_head_bwd" in seq_py
    assert torch.equal(got[0], want["energy"].detach()) and torch.equal(got[2], want["forces"].detach())


def test_compile_model_scripts_saves_reloads_and_reproduces(tmp_path):
    """run/jit_script.py:28-86: torch.jit.script of the LAMMPS front end, saved with `_extra_files`, reloaded, evaluated: the
    eager XPaiNNLMP's energies and forces bit for bit; the GROMACS front end's energy and its autograd forces likewise."""
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.interface import XPaiNNGMX, XPaiNNLMP
    from xequinet_amd.interface.scripted import compile_model

    dtype = torch.float32
    lmp, _ = _twin(XPaiNNLMP, dtype, unit_style="real")
    path = str(tmp_path / "xpainn-lmp-real.jit")
    compile_model(lmp, mode="lmp", unit_style="real", output_file=path)
    extra = {"cutoff_radius": "", "n_species": "", "periodic_table": "", "fusion_strategy": ""}
    loaded = torch.jit.load(path, _extra_files=extra)
    assert float(extra["cutoff_radius"]) == pytest.approx(lmp.cutoff_radius) and int(extra["n_species"]) == 87
    assert extra["periodic_table"].decode().split()[:3] == ["X", "H", "He"]
    pos, z, ptr = syn.synth_qm9_batch(1, seed=3)
    b = NeighborTransform(5.0)(XequiBatch(P._t(pos, dtype), P._t(z), P._t(ptr)))
    data = {"pos": b.pos, "atomic_numbers": b.atomic_numbers, "edge_index": b.edge_index}
    with torch.enable_grad():
        want = lmp(dict(data), compute_forces=True, compute_virial=False)
    got = loaded(dict(data), True, False)
    assert set(got) == {"energy", "atomic_energies", "forces"}
    assert torch.equal(got["energy"], want["energy"].detach()) and torch.equal(got["forces"], want["forces"].detach())

    gmx, _ = _twin(XPaiNNGMX, dtype)
    path = str(tmp_path / "xpainn-gmx.pt")
    compile_model(gmx, mode="gmx", output_file=path)
    loaded = torch.jit.load(path)
    p_nm = (b.pos / 10.0).detach()
    pa = p_nm.clone().requires_grad_()
    ea = gmx(pa, b.atomic_numbers)
    (fa,) = torch.autograd.grad(ea.sum(), pa)
    pb = p_nm.clone().requires_grad_()
    eb = loaded(pb, b.atomic_numbers)
    (fb,) = torch.autograd.grad(eb.sum(), pb)
    assert torch.equal(ea.detach(), eb.detach())
    np.testing.assert_allclose(fb.cpu().numpy(), fa.cpu().numpy(), rtol=0, atol=2e-6 * float(fa.abs().max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scripted_gromacs_model_searches_periodic_boxes(dtype, tmp_path):
    """interface/jit_model.py:183-214 scripted: `single_radius_graph` runs INSIDE the model for a periodic box.  The registered
    operator xeq::radius_graph_pbc gives the reference's list bit for bit (the reference-generated fixture of the 192-atom
    water box; the Python search on a 1 536-atom box and on the triclinic fixture's cell), and the scripted, saved and
    reloaded GROMACS model returns the Python XPaiNNGMX's energy bit for bit, its autograd forces to rounding of the unit
    factor, on all three."""
    from xequinet_amd.data import single_radius_graph
    from xequinet_amd.interface import XPaiNNGMX
    from xequinet_amd.interface.scripted import compile_model, load_torch_library

    load_torch_library()
    npdt = np.float32 if dtype == torch.float32 else np.float64
    nm = FACTOR[("nm", "Angstrom")]
    gmx, _ = _twin(XPaiNNGMX, dtype)
    path = str(tmp_path / "xpainn-gmx-pbc.pt")
    compile_model(gmx, mode="gmx", output_file=path)
    loaded = torch.jit.load(path)

    a = P._load("radius_graph_pbc_water192.npz")
    f = P._load("single_radius_graph_water192.npz")
    _, z192, _, _ = syn.synth_water_box(4, seed=5)
    pos512, z512, _, cell512 = syn.make_workload("water_512", seed=0)
    t = P._load("radius_graph_pbc_triclinic40.npz")
    rng = np.random.default_rng(3)
    cases = [("water_192", a["pos"], z192, a["cell"][0], [True, True, True], f),
             ("water_512", pos512, z512, np.asarray(cell512).reshape(-1, 3, 3)[0], [True, True, True], None),
             ("triclinic40", t["pos"], rng.choice([1, 6, 8], size=len(t["pos"])), t["cell"][0], [bool(v) for v in np.asarray(t["pbc"]).reshape(-1, 3)[0]], None),
             ("slab (open along z)", a["pos"], z192, a["cell"][0], [True, True, False], None)]
    for name, pos, z, cell, pbc, fixture in cases:
        pos_t, cell_t = P._t(pos.astype(npdt)), P._t(cell.astype(npdt))
        pbc_t = torch.tensor(pbc, device=DEV)
        ei, co, rowptr = torch.ops.xeq.radius_graph_pbc(pos_t, cell_t, pbc_t, 5.0)
        ei_py, co_py, rp_py = single_radius_graph(pos_t, pbc_t, cell_t, 5.0, return_rowptr=True)
        assert torch.equal(ei, ei_py) and torch.equal(co, co_py) and torch.equal(rowptr, rp_py), name
        assert ei.shape[1] > 0 and ei.dtype == torch.int64 and co.dtype == dtype, name
        if fixture is not None and dtype == torch.float32:   # the fixture was generated by the reference in its default dtype
            np.testing.assert_array_equal(ei.cpu().numpy(), fixture["edge_index"])
            np.testing.assert_array_equal(co.cpu().numpy(), fixture["cell_offsets"])
        zt = P._t(np.asarray(z).astype(np.int64))
        box = cell_t / nm
        pa = (pos_t / nm).detach().clone().requires_grad_()
        ea = gmx(pa, zt, box, pbc_t)
        (fa,) = torch.autograd.grad(ea.sum(), pa)
        pb = (pos_t / nm).detach().clone().requires_grad_()
        eb = loaded(pb, zt, box, pbc_t)
        (fb,) = torch.autograd.grad(eb.sum(), pb)
        assert torch.equal(ea.detach(), eb.detach()), (name, ea, eb)
        np.testing.assert_allclose(fb.cpu().numpy(), fa.cpu().numpy(), rtol=0, atol=2e-6 * float(fa.abs().max()), err_msg=name)


def test_native_operator_on_a_stream_of_new_topologies_matches_oracle():
    """One operator call per batch, every batch with another edge count (nothing to replay): energies / forces against the
    fp64 oracle."""
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.interface.scripted import XPaiNNNative

    model, oracle = P._build(torch.float64)
    native = XPaiNNNative(model)
    seen = set()
    for seed in (1, 2, 3):
        pos, z, ptr = syn.synth_qm9_batch(5 + seed, seed=40 + seed)
        b = NeighborTransform(5.0)(XequiBatch(P._t(pos, torch.float64), P._t(z), P._t(ptr)))
        seen.add(b.edge_index.shape[1])
        out = native(b.pos, b.atomic_numbers, b.edge_index, b.ptr, None, None, True, True, True, False)
        want = oracle(_oracle_in(pos, z, ptr, b.edge_index.cpu().numpy()), compute_forces=True)
        np.testing.assert_allclose(out[0].cpu().numpy(), want["energy"].numpy(), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(out[2].cpu().numpy(), want["forces"].numpy(), rtol=0, atol=1e-9)
    assert len(seen) == 3


def test_native_operator_never_reuses_the_weight_packs_of_a_dead_model():
    """The operator caches matrix-core weight copies per parameter tensor.  A deleted model's parameter addresses are handed to the
    next model of the same shapes (same version counters): the cache must notice that its owners died."""
    import gc

    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.interface.scripted import XPaiNNNative
    from xequinet_amd.nn import resolve_model

    pos, z, ptr = syn.synth_qm9_batch(6, seed=77)
    b = NeighborTransform(5.0)(XequiBatch(P._t(pos, torch.float32), P._t(z), P._t(ptr)))
    energies = []
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        model = resolve_model("xpainn").eval().requires_grad_(False).to(DEV)
        native = XPaiNNNative(model)
        got = native(b.pos, b.atomic_numbers, b.edge_index, b.ptr, None, None, True, True, True, False)
        with torch.enable_grad():
            want = model(b.to_dict(), compute_forces=True, compute_virial=False)
        assert torch.equal(got[0], want["energy"].detach()) and torch.equal(got[2], want["forces"].detach()), f"model {seed}"
        energies.append(got[0].clone())
        del model, native, got, want
        gc.collect()
        torch.cuda.empty_cache()
    assert not torch.equal(energies[0], energies[1]) and not torch.equal(energies[1], energies[2])


def test_replay_follows_a_weight_update():
    """A captured graph reads packed weight copies made at capture time; an in-place update of the parameters drops the graphs
    (runtime._Weights, which GraphedModel inherits), so replay and the eager model keep agreeing."""
    from xequinet_amd import runtime
    from xequinet_amd.data import NeighborTransform, XequiBatch, synthetic as syn
    from xequinet_amd.nn import resolve_model

    torch.manual_seed(0)
    model = resolve_model("xpainn", action_blocks=2).eval().requires_grad_(False).to("cuda")
    pos, z, ptr = syn.synth_qm9_batch(8, seed=4)
    batch = NeighborTransform(5.0)(XequiBatch(torch.tensor(pos, dtype=torch.float32, device="cuda"), torch.tensor(z, device="cuda"),
                                              torch.tensor(ptr, device="cuda")))
    g = runtime.GraphedModel(model, tune_gemms=False)

    def both():
        r = {k: v.clone() for k, v in g(batch.to_dict()).items()}
        with torch.enable_grad():
            e = model(batch.to_dict(), compute_forces=True, compute_virial=False)
        return r, e

    r0, e0 = both()
    assert torch.equal(r0["forces"], e0["forces"]) and g.captures == 1
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.05)
    r1, e1 = both()
    assert g.captures == 2
    assert torch.equal(r1["forces"], e1["forces"]) and not torch.equal(r1["forces"], r0["forces"])
    r2, _ = both()
    assert g.captures == 2 and torch.equal(r2["forces"], r1["forces"])


def test_lammps_replay_reuses_an_unchanged_neighbour_list():
    """XPaiNNLMP(replay=True): when the engine hands over the same list again (positions moved), the sorted views held by the
    captured graph are reused (GraphedModel.reuse_unchanged_topology); a different list of the same length rebuilds them.
    Every step equals the eager model."""
    from xequinet_amd.cluster import radius_graph
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.interface import XPaiNNLMP

    torch.manual_seed(0)
    pos, z, _ = syn.synth_aspirin()
    p0 = torch.tensor(pos, dtype=torch.float32, device="cuda")
    zz = torch.tensor(z, device="cuda")
    kw = dict(unit_style="metal", action_blocks=2)
    torch.manual_seed(1)
    fast = XPaiNNLMP(replay=True, tune_gemms=False, **kw).eval().requires_grad_(False).to("cuda")
    torch.manual_seed(1)
    ref = XPaiNNLMP(replay=False, **kw).eval().requires_grad_(False).to("cuda")
    ei = radius_graph(p0, 5.0, ptr=torch.tensor([0, len(z)], device="cuda"))
    perm = torch.randperm(ei.shape[1], device="cuda")
    lists = [ei, ei.clone(), ei.clone(), ei[:, perm].contiguous(), ei[:, perm].contiguous(), ei]     # same, same, same, reordered, same, back
    g = torch.Generator(device="cuda").manual_seed(3)
    built = []
    import xequinet_amd.ops as ops_mod
    orig = ops_mod.EdgeGraph.__init__

    def counting(self, *a, **k):
        built.append(1)
        return orig(self, *a, **k)

    ops_mod.EdgeGraph.__init__ = counting
    try:
        for step, e in enumerate(lists):
            p = p0 + 0.02 * torch.randn(p0.shape, device="cuda", generator=g)
            n_before = len(built)
            with torch.enable_grad():
                a = fast({"pos": p.clone(), "atomic_numbers": zz, "edge_index": e}, True, False)
            n_fast = len(built) - n_before
            with torch.enable_grad():
                b = ref({"pos": p.clone(), "atomic_numbers": zz, "edge_index": e}, True, False)
            assert torch.allclose(a["energy"], b["energy"], rtol=1e-5, atol=1e-5), step
            assert (a["forces"] - b["forces"]).abs().max().item() <= 2e-4, step
            if step in (1, 2, 4):
                assert n_fast == 0, f"step {step}: the unchanged list was rebuilt"
            if step in (3, 5):
                assert n_fast >= 1, f"step {step}: a changed list must be rebuilt"
    finally:
        ops_mod.EdgeGraph.__init__ = orig


def test_ase_calculator_native_operator_gives_the_module_numbers():
    """XequiCalculator(native=True): the evaluation is one registered operator (xeq::xpainn_eval) -- same kernels in the same
    order as the Python modules, so energy, atomic energies, forces and stress are bit-identical; molecule and periodic box."""
    import time
    from xequinet_amd.interface import XequiCalculator
    from xequinet_amd.interface.ase_calculator import _HAVE_ASE

    if _HAVE_ASE:
        pytest.skip("duck-typed Atoms stand-in is for images without ASE")
    model, _ = P._build(torch.float32)
    plain = XequiCalculator(model=model, dtype="float32")
    fast = XequiCalculator(model=model, dtype="float32", native=True)
    pos, z, _ = syn.synth_aspirin()
    f = P._load("radius_graph_pbc_water192.npz")
    _, zw, _, _ = syn.synth_water_box(4, seed=5)
    cell = f["cell"][0].astype(np.float64)
    systems = [(_Atoms(pos, z), ["energy", "forces"]), (_Atoms(f["pos"].astype(np.float64), zw, cell, (True, True, True)), None)]
    for atoms, props in systems:
        plain.calculate(atoms, props)
        fast.calculate(atoms, props)
        assert fast._native is not None
        assert set(plain.results) == set(fast.results)
        for k in plain.results:
            assert np.array_equal(np.asarray(plain.results[k]), np.asarray(fast.results[k])), k
    # and it is the faster path for a small molecule (host-bound either way; generous margin)
    atoms = systems[0][0]
    def timed(calc):
        for _ in range(3):
            calc.calculate(atoms, ["energy", "forces"])
        t0 = time.perf_counter()
        for _ in range(20):
            calc.calculate(atoms, ["energy", "forces"])
        return (time.perf_counter() - t0) / 20
    t_plain, t_fast = timed(plain), timed(fast)
    print(f"ASE-style step on aspirin: modules {t_plain * 1e3:.2f} ms, native operator {t_fast * 1e3:.2f} ms")
    assert t_fast < t_plain


def test_lammps_model_native_operator_option():
    """XPaiNNLMP(native=True) against the same model through the Python modules: bit-identical energies and forces."""
    from xequinet_amd.cluster import radius_graph
    from xequinet_amd.interface import XPaiNNLMP

    pos, z, _ = syn.synth_aspirin()
    p = torch.tensor(pos, dtype=torch.float32, device="cuda")
    zz = torch.tensor(z, device="cuda")
    ei = radius_graph(p, 5.0, ptr=torch.tensor([0, len(z)], device="cuda"))
    torch.manual_seed(1)
    a = XPaiNNLMP(unit_style="real", native=True, action_blocks=2).eval().requires_grad_(False).to("cuda")
    torch.manual_seed(1)
    b = XPaiNNLMP(unit_style="real", action_blocks=2).eval().requires_grad_(False).to("cuda")
    for _ in range(2):
        with torch.enable_grad():
            ra = a({"pos": p.clone(), "atomic_numbers": zz, "edge_index": ei}, True, False)
            rb = b({"pos": p.clone(), "atomic_numbers": zz, "edge_index": ei}, True, False)
        assert a._native is not None
        assert torch.equal(ra["energy"], rb["energy"]) and torch.equal(ra["forces"], rb["forces"])
    assert "_native" not in dict(a.named_modules()) and len(a.state_dict()) == len(b.state_dict())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_gromacs_model_whole_step_graph_follows_a_trajectory(dtype, monkeypatch):
    """XPaiNNGMX(replay=True, whole_step=True): neighbour search + evaluation as ONE captured graph over capacity-sized edge arrays
    (runtime.GraphedStepPBC).  A short trajectory (positions move, the edge count with them; the box breathes): every step's energy
    equals the eager model's bit for bit and the forces to the unit factor's rounding, on one capture; a capacity that is too small
    re-captures with more room and gives the same numbers; another image count per axis (a much smaller box) re-captures."""
    from xequinet_amd.interface import XPaiNNGMX

    if dtype == torch.float32:   # `auto` picks the family by the edge count it knows: the true one (eager) or the capacity (graph);
        monkeypatch.setenv("XEQ_MESSAGE_IMPL", "wq")   # near 4 096 edges they could differ, and with them the last bits
    npdt = np.float32 if dtype == torch.float32 else np.float64
    nm = FACTOR[("nm", "Angstrom")]
    eager, _ = _twin(XPaiNNGMX, dtype)
    fast, _ = _twin(XPaiNNGMX, dtype, replay=True, whole_step=True, tune_gemms=False)
    fast.load_state_dict(eager.state_dict())
    a = P._load("radius_graph_pbc_water192.npz")
    _, z192, _, _ = syn.synth_water_box(4, seed=5)
    pos512, z512, _, cell512 = syn.make_workload("water_512", seed=0)
    pos81, z81, _, cell81 = syn.synth_water_box(3, seed=2)
    rng = np.random.default_rng(8)
    cases = [("water_192", a["pos"], z192, a["cell"][0], [True, True, True]),
             ("water_512", pos512, z512, np.asarray(cell512).reshape(-1, 3, 3)[0], [True, True, True]),
             ("81 atoms, box < 2 cutoffs", pos81, z81, np.asarray(cell81).reshape(-1, 3, 3)[0], [True, True, True]),
             ("slab (open along z)", a["pos"], z192, a["cell"][0], [True, True, False])]
    for name, pos0, z, cell0, pbc in cases:
        z_t, pbc_t = P._t(np.asarray(z).astype(np.int64)), torch.tensor(pbc, device=DEV)
        fast._step_graph = None
        counts = []
        for step in range(5):
            pos = pos0 + 0.05 * step * rng.normal(size=pos0.shape)
            cell = cell0 * (1.0 + 0.002 * step)                                   # the box breathes: same image counts, new tables
            outs = []
            for model in (eager, fast):
                x = P._t((pos / nm).astype(npdt)).requires_grad_(True)
                e = model(x, z_t, P._t((cell / nm).astype(npdt)), pbc_t)
                (g,) = torch.autograd.grad(e.sum(), x)
                outs.append((e.detach().clone(), g.clone()))
            assert torch.equal(outs[0][0], outs[1][0]), (name, step)
            scale = outs[0][1].abs().max().item()
            assert (outs[0][1] - outs[1][1]).abs().max().item() <= 16 * torch.finfo(dtype).eps * scale, (name, step)   # (two unit factors applied in another order)
            counts.append(int(fast._step_graph.outputs["n_edges"].item()))
        assert fast._step_graph.captures == 1, name
        assert len(set(counts)) > 1, (name, counts)                              # the edge count did move under the one graph
        # a capacity far too small: cut lists are detected, the graph re-captured with more room, same numbers
        from xequinet_amd.runtime import GraphedStepPBC
        from xequinet_amd.interface.md_model import _Core
        small = GraphedStepPBC(_Core(fast), len(pos0), 64, cutoff=fast.cutoff_radius)
        fast._step_graph = small
        x = P._t((pos / nm).astype(npdt)).requires_grad_(True)
        e = fast(x, z_t, P._t((cell / nm).astype(npdt)), pbc_t)
        assert torch.equal(e.detach(), outs[0][0]) and small.captures >= 2 and small.n_edges >= counts[-1], name
    # a box of another size class: more images per axis -> another table, another graph
    g = fast._step_graph
    caps = g.captures
    x = P._t((a["pos"] / nm).astype(npdt)).requires_grad_(True)
    half = P._t((a["cell"][0] * 0.3 / nm).astype(npdt))
    e1 = fast(x, P._t(np.asarray(z192).astype(np.int64)), half, torch.tensor([True, True, False], device=DEV))
    e0 = eager(x, P._t(np.asarray(z192).astype(np.int64)), half, torch.tensor([True, True, False], device=DEV))
    assert fast._step_graph.captures > caps and torch.equal(e0.detach(), e1.detach())


def test_gromacs_model_whole_step_graph_without_a_box():
    """No box, no periodic axis (an isolated molecule under GROMACS' NNPot): the whole-step graph searches with one image (rep 0 on
    every axis) and returns the eager model's energy bit for bit, forces to the unit factors' rounding, along a short trajectory."""
    from xequinet_amd.interface import XPaiNNGMX

    dtype = torch.float32
    nm = FACTOR[("nm", "Angstrom")]
    eager, _ = _twin(XPaiNNGMX, dtype)
    fast, _ = _twin(XPaiNNGMX, dtype, replay=True, whole_step=True, tune_gemms=False)
    fast.load_state_dict(eager.state_dict())
    pos0, z, _ = syn.synth_aspirin()
    z_t = P._t(np.asarray(z).astype(np.int64))
    rng = np.random.default_rng(4)
    for step in range(4):
        pos = pos0 + 0.03 * step * rng.normal(size=pos0.shape)
        outs = []
        for model in (eager, fast):
            x = P._t((pos / nm).astype(np.float32)).requires_grad_(True)
            e = model(x, z_t, None, None)
            (g,) = torch.autograd.grad(e.sum(), x)
            outs.append((e.detach().clone(), g.clone()))
        assert torch.equal(outs[0][0], outs[1][0]), step
        assert (outs[0][1] - outs[1][1]).abs().max().item() <= 16 * torch.finfo(dtype).eps * outs[0][1].abs().max().item(), step
    assert fast._step_graph.captures == 1


def test_lammps_replay_on_an_unchanged_list_skips_the_plan_rebuild_and_changes_no_bit():
    """runtime.GraphedModel keeps a second captured graph without the walk-plan rebuild for replays on an unchanged list (a periodic
    192-atom box: the wq message kernels and their plans).  Same positions through the first graph (capture), the plan-free graph
    (second and third call) and a model that rebuilds every time: the same bits; moved positions: equal to the eager model."""
    from xequinet_amd.data import single_radius_graph
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.interface import XPaiNNLMP

    pos, z, _, cell = syn.synth_water_box(4, seed=5)
    p0 = torch.tensor(pos, dtype=torch.float32, device="cuda")
    zz = torch.tensor(z, device="cuda")
    c = torch.tensor(cell[0], dtype=torch.float32, device="cuda")
    pbc = torch.tensor([True, True, True], device="cuda")
    ei, co = single_radius_graph(p0, pbc, c, 5.0)
    kw = dict(unit_style="metal")
    torch.manual_seed(1)
    fast = XPaiNNLMP(replay=True, tune_gemms=False, **kw).eval().requires_grad_(False).to("cuda")
    torch.manual_seed(1)
    ref = XPaiNNLMP(replay=False, **kw).eval().requires_grad_(False).to("cuda")

    def run(m, p):
        with torch.enable_grad():
            out = m({"pos": p.clone(), "atomic_numbers": zz, "edge_index": ei, "cell": c[None], "cell_offsets": co, "pbc": pbc[None]}, True, False)
        return out["energy"].clone(), out["forces"].clone()

    e1, f1 = run(fast, p0)           # capture + the graph with the plan rebuild
    e2, f2 = run(fast, p0)           # captures and replays the plan-free graph
    e3, f3 = run(fast, p0)           # replays it
    assert fast._replay.captures == 1 and getattr(fast._replay, "captures_same_list", 0) == 1
    assert torch.equal(e1, e2) and torch.equal(f1, f2) and torch.equal(e1, e3) and torch.equal(f1, f3)
    g = torch.Generator(device="cuda").manual_seed(3)
    p1 = p0 + 0.02 * torch.randn(p0.shape, device="cuda", generator=g)
    e4, f4 = run(fast, p1)
    e5, f5 = run(ref, p1)
    assert torch.allclose(e4, e5, rtol=1e-5, atol=1e-5) and (f4 - f5).abs().max().item() <= 2e-4
    assert not torch.equal(f4, f1)


def test_any_differs_compares_several_pairs_in_one_launch():
    """ops.any_differs (xeq_compare_many): what GraphedModel asks about the engine's list -- repeated calls (the flag is never cleared:
    every call hands a new generation), a difference in any pair, in the last word, shape / dtype mismatches, empty and aliased pairs."""
    from xequinet_amd import ops

    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randint(0, 1000, (2, 4097), device="cuda", generator=g)
    b = torch.randn(333, 3, device="cuda", generator=g)
    c = torch.tensor([0, 21], device="cuda")
    for _ in range(3):
        assert not ops.any_differs([(a, a.clone()), (b, b.clone()), (c, c.clone())])
    a2 = a.clone()
    a2[1, -1] += 1
    assert ops.any_differs([(a, a2), (b, b.clone())]) and ops.any_differs([(b, b.clone()), (a, a2)])
    assert not ops.any_differs([(a, a.clone())])                      # and clean again afterwards
    b2 = b.clone()
    b2[0, 0] = b2[0, 0] + 1.0
    assert ops.any_differs([(a, a.clone()), (b, b2)])
    assert ops.any_differs([(a, a[:, :-1])]) and ops.any_differs([(c, c.to(torch.int32))])
    assert not ops.any_differs([(a, a), (torch.empty(0, device="cuda"), torch.empty(0, device="cuda"))])
    assert ops.any_differs([(a.t(), a2.t())]) and not ops.any_differs([(a.t(), a.clone().t())])    # non-contiguous: torch.equal


@pytest.mark.parametrize("n_mol", [24, 400])
def test_native_operator_packs_follow_the_weights(n_mol):
    """xeq::xpainn_eval keeps no packed copy past a change of a weight it was made from: one weight per pack cache of csrc/xeq_torch.cpp is
    modified in place, and the next evaluation equals, bit for bit, one on freshly allocated tensors with the same values.  The parameters
    are XPaiNNNative's, each in a tensor of its own (the views of the module's flat buffer share ONE version counter: a change of any
    of them would make every cache miss, and the test would not tell the caches apart).  24 molecules: the chain of small node kernels
    (MLP, linear, U / V and element-table packs); 400: the fused node blocks and the wq message kernels (their weight programs)."""
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.interface.scripted import XPaiNNNative

    model, _ = P._build(torch.float32)
    native = XPaiNNNative(model)
    pos, z, ptr = syn.synth_qm9_batch(n_mol, seed=13)
    data = NeighborTransform(5.0)(XequiBatch(P._t(pos, torch.float32), P._t(z), P._t(ptr))).to_dict()
    prm = [native.flat[o:o + math.prod(shape)].view(shape).clone() for o, shape in zip(native.offsets, native.shapes)]

    def evaluate(params):
        return torch.ops.xeq.xpainn_eval(data["pos"].detach(), data["atomic_numbers"], data["edge_index"], data["ptr"], None, None, params,
                                         native.iparams, native.fparams, True, True, True, False, None, None)

    evaluate(prm)
    blk0, blk1, head = 5, 5 + 27, 5 + 27 * native.iparams[5]      # the parameter layout of csrc/xeq_torch.cpp
    sites = {"embedding weight (element table front)": 1, "block 0 scalar_mlp.0.bias (element table front)": blk0 + 1,
             "block 1 scalar_mlp.2.weight (MLP pack / node block program)": blk1 + 2, "block 1 rbf_lin.weight (wq weight pack)": blk1 + 4,
             "block 0 U|V pack l=1 (U / V pack / node block program)": blk0 + 11, "block 0 U|V bias (U / V pack / node block bias)": blk0 + 13,
             "block 0 dot_lin.weight (linear pack / node block program)": blk0 + 14, "block 0 update_mlp.0.weight (MLP pack / node block program)": blk0 + 15,
             "block 0 update_mlp.2.bias": blk0 + 18, "head.0.weight (linear pack)": head, "head.0.bias (linear pack)": head + 1}
    for name, i in sites.items():
        with torch.no_grad():
            prm[i].mul_(1.25).add_(0.01)
        got, want = evaluate(prm), evaluate([t.clone() for t in prm])
        for k in range(3):
            assert torch.equal(got[k], want[k]), f"after a change of {name}: output {k} differs by {(got[k] - want[k]).abs().max().item():.2e}"
