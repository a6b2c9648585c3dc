"""PaiNN on the MI355X: the kernels of csrc/xeq_painn.hip and the model built from them against the f64 oracle
(tests/painn_oracle.py, pinned to the reference's numbers by tests/test_painn_host.py).

Bounds -- the project's rule (tests/test_gpu_electronic.py::_compare): energy 1e-5 max|E| + 1e-4; forces max(1e-4, 1.5 err32); virial
the same form scaled by max(1, max|virial|); err32 is the distance of the ORACLE run in f32 from the oracle in f64 on the same inputs.
Kernel-level outputs use the same form: max(1e-4 max(1, max|ref|), 1.5 err32)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import guard_bands, painn_oracle as po, parity_record
from xequinet_amd import keys, lib
from xequinet_amd.data import NeighborTransform, XequiBatch
from xequinet_amd.data import synthetic as syn
from xequinet_amd.nn import resolve_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
LAUNCHES_PER_EVALUATION = 37   # DESIGN.md, "PaiNN": energy + forces of the 3-block model, neighbour list given


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    model = resolve_model("painn", **kw)
    with torch.no_grad():   # an energy head that is not nearly flat
        for p in model.mods["output_energy"].parameters():
            p.mul_(2.0)
    return model.to(DEV).eval().requires_grad_(False)


def _batch(pos, z, ptr, cutoff, cell=None):
    kw = {} if cell is None else {"cell": torch.tensor(cell, dtype=torch.float32), "pbc": torch.tensor([[True, True, True]] * (len(ptr) - 1))}
    b = XequiBatch(torch.tensor(pos, dtype=torch.float32), torch.tensor(z), torch.tensor(ptr), **kw).to(DEV)
    return NeighborTransform(cutoff)(b).to_dict()


def _eval(model, data, virial=False):
    with torch.enable_grad():
        out = model(dict(data), compute_forces=True, compute_virial=virial)
    return {k: v.detach() for k, v in out.items()}


def _oracle(model, data, virial, dtype):
    sd = po.cast({k: v.detach().cpu().double() for k, v in model.state_dict().items()}, dtype)
    c = lambda k: data[k].detach().cpu()
    cell = c("cell").to(dtype) if "cell" in data else None
    off = c("cell_offsets").to(dtype) if "cell" in data else None
    n_blocks = sum(1 for k in model.mods if k.startswith("message_"))
    return po.model(sd, c("atomic_numbers").long(), c("pos").to(dtype), c("edge_index"), c("batch").long(), c("ptr").numel() - 1, n_blocks,
                    model.cutoff_radius, cell=cell, cell_offsets=off, virial=virial)


def _compare(model, data, virial=False, tag=""):
    got = _eval(model, data, virial)
    ref, ref32 = _oracle(model, data, virial, torch.float64), _oracle(model, data, virial, torch.float32)
    e, e_ref = got["energy"].cpu().double(), ref["energy"].detach()
    de = float((e - e_ref).abs().max())
    err32 = float((ref32["forces"].double() - ref["forces"]).abs().max())
    df = float((got["forces"].cpu().double() - ref["forces"]).abs().max())
    rec = {"test": "painn:" + tag, "dE": de, "dF": df, "err32_F": err32, "max_F": float(ref["forces"].abs().max())}
    if virial:
        verr32 = float((ref32["virial"].double() - ref["virial"]).abs().max())
        dv = float((got["virial"].cpu().double() - ref["virial"]).abs().max())
        rec.update(dV=dv, err32_V=verr32)
    parity_record.add(rec)
    print(rec)
    assert torch.isfinite(got["forces"]).all()
    assert de <= float(1e-5 * e_ref.abs().max() + 1e-4), rec
    assert df <= max(1e-4, 1.5 * err32), rec
    if virial:
        assert dv <= max(1e-4 * max(1.0, float(ref["virial"].abs().max())), 1.5 * verr32), rec
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------- kernels
def _fixture_model():
    f = np.load(os.path.join(GOLDEN, "painn_model_f64.npz"))
    shapes = json.load(open(os.path.join(GOLDEN, "painn_keys.json")))["gfn2-xtb"]
    model = resolve_model("painn")
    sd = model.state_dict()
    sd.update({"mods." + k: v.float() for k, v in po.seeded_weights(shapes, int(f["seed"])).items()})
    model.load_reference_state_dict(sd)
    return f, model.to(DEV).eval().requires_grad_(False)


def _bound(ref, ref32):
    return max(1e-4 * max(1.0, float(ref.abs().max())), 1.5 * float((ref32.double() - ref).abs().max()))


def _fixture_states(f, model, dtype):
    """Oracle node features (s, x) in front of message_1 and update_1, from the reference's inputs."""
    sd = po.cast({k[len("mods."):]: v.detach().cpu().double() for k, v in model.state_dict().items()}, dtype)
    pos, ei = torch.tensor(f["mol_pos"]).to(dtype), torch.tensor(f["mol_edge_index"])
    vec = po.edge_vectors(pos, ei)
    rbf, fcut, u = po.radial(vec, sd["embedding.rbf.freq"], 5.0)
    s = po.embedding(torch.tensor(f["mol_z"]), sd)
    x = torch.zeros((s.shape[0], 3, 128), dtype=dtype)
    s, x = po.message(s, x, rbf, fcut, u, ei, sd, "message_0.")
    s, x = po.update(s, x, sd, "update_0.")
    return sd, vec, (rbf, fcut, u), ei, s, x


def test_message_and_update_kernels_against_the_reference_fixture():
    """message_1 / update_1 of the fixture model (x != 0) forward and reverse, fed the oracle's f64 state rounded to f32, against oracle
    autograd (the oracle itself is pinned to painn_model_f64.npz by tests/test_painn_host.py)."""
    from xequinet_amd.nn import painn
    from xequinet_amd.nn.basic import edge_graph

    f, model = _fixture_model()
    sd, vec, (rbf, fcut, u), ei, s0, x0 = _fixture_states(f, model, torch.float64)
    sd32, vec32, (rbf32, fcut32, u32), _, _, _ = _fixture_states(f, model, torch.float32)
    emb = model.mods["embedding"]
    data = {keys.POSITIONS: torch.tensor(f["mol_pos"], dtype=torch.float32, device=DEV), keys.EDGE_INDEX: ei.to(DEV)}
    graph = edge_graph(data)
    g_s_out, g_x_out = torch.randn(s0.shape, dtype=torch.float64), torch.randn(x0.shape, dtype=torch.float64)

    def run_oracle(s, x, vec, rbf_fcut_u, sd, which):
        s, x, vec = s.clone().requires_grad_(), x.clone().requires_grad_(), vec.clone().requires_grad_()
        if which == "message":
            out = po.message(s, x, *po.radial(vec, sd["embedding.rbf.freq"], 5.0), ei, sd, "message_1.")
            wrt = [s, x, vec]
        else:
            out = po.update(s, x, sd, "update_1.")
            wrt = [s, x]
        grads = torch.autograd.grad(out, wrt, [g_s_out.to(s.dtype), g_x_out.to(s.dtype)])
        return [o.detach() for o in out] + list(grads)

    for which in ("message", "update"):
        ref = run_oracle(s0, x0, vec, None, sd, which)
        ref32 = run_oracle(s0.float(), x0.float(), vec.float(), None, sd32, which)
        with guard_bands.guard_allocations():
            s = s0.float().to(DEV).requires_grad_()
            x = x0.float().to(DEV).requires_grad_()
            v = vec.float().to(DEV).requires_grad_()
            with torch.enable_grad():
                if which == "message":
                    out = painn.MessageFn.apply(s, x, v, model.mods["message_1"], graph, emb.rbf, emb.cutoff_fn, None, False)
                    wrt = [s, x, v]
                else:
                    out = painn.UpdateFn.apply(s, x, model.mods["update_1"], True)
                    wrt = [s, x]
                grads = torch.autograd.grad(out, wrt, [g_s_out.float().to(DEV), g_x_out.float().to(DEV)])
            got = [o.detach() for o in out] + list(grads)
            torch.cuda.synchronize()
        names = ["s_out", "x_out", "g_s", "g_x", "g_vec"]
        for name, a, r, r32 in zip(names, got, ref, ref32):
            d = float((a.cpu().double() - r).abs().max())
            parity_record.add({"test": f"painn:kernel:{which}:{name}", "err": d, "bound": _bound(r, r32)})
            print(which, name, d, _bound(r, r32))
            assert torch.isfinite(a).all() and d <= _bound(r, r32), (which, name, d, _bound(r, r32))


# ------------------------------------------------------------------------------------------------------------------------ model
def test_fixture_model_against_the_reference_numbers():
    """The reference's own energies-through-a-linear-readout are not what the model's head computes; its per-block node scalars are:
    compare the scalars behind the last block with painn_model_f64.npz."""
    f, model = _fixture_model()
    ptr = f["mol_ptr"]
    data = {"pos": torch.tensor(f["mol_pos"], dtype=torch.float32, device=DEV), "atomic_numbers": torch.tensor(f["mol_z"]).to(DEV),
            "edge_index": torch.tensor(f["mol_edge_index"]).to(DEV), "ptr": torch.tensor(ptr).to(DEV),
            "batch": torch.tensor(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))).to(DEV)}
    seen = []
    model.mods["update_2"].register_forward_hook(lambda mod, inp, out: seen.append(out[keys.NODE_INVARIANT].detach().clone()))
    _compare(model, data, tag="fixture_mol")
    sd32 = {k: v.detach().cpu().float() for k, v in model.state_dict().items()}
    z, ei = torch.tensor(f["mol_z"]), torch.tensor(f["mol_edge_index"])
    vec32 = po.edge_vectors(torch.tensor(f["mol_pos"]).float(), ei)
    s32, x32 = po.blocks(z, vec32, ei, sd32, 3, 5.0, "mods.")
    ref = torch.tensor(f["mol_s_blocks"][2])
    d = float((seen[0].cpu().double() - ref).abs().max())
    assert d <= _bound(ref, s32), (d, _bound(ref, s32))
    # the message and update kernels of the first two blocks alone, and the vectors behind the last block (formed on request)
    s32_1, _ = po.blocks(z, vec32, ei, sd32, 2, 5.0, "mods.")
    model.mods["update_2"].equivariant_output_unused = False
    mid, last_x = [], []
    model.mods["update_1"].register_forward_hook(lambda mod, inp, out: mid.append(out[keys.NODE_INVARIANT].detach().clone()))
    model.mods["update_2"].register_forward_hook(lambda mod, inp, out: last_x.append(out[keys.NODE_EQUIVARIANT].detach().clone()))
    _eval(model, data)
    for name, got, want, want32 in (("s_block_1", mid[0], torch.tensor(f["mol_s_blocks"][1]), s32_1),
                                    ("x_last", last_x[0], torch.tensor(f["mol_x_last"]), x32)):
        d = float((got.cpu().double() - want).abs().max())
        parity_record.add({"test": "painn:fixture:" + name, "err": d, "bound": _bound(want, want32)})
        assert got.shape == want.shape and d <= _bound(want, want32), (name, d, _bound(want, want32))


def test_qm9_batch_against_oracle():
    model = _model(1)
    pos, z, ptr = syn.synth_qm9_batch(16, seed=3)
    with guard_bands.guard_allocations():
        _compare(model, _batch(pos, z, ptr, model.cutoff_radius), tag="qm9_16")
        torch.cuda.synchronize()


def test_aspirin_few_rows_against_oracle():
    model = _model(2)
    pos, z, ptr = syn.synth_aspirin()
    assert len(z) <= lib.load().xeq_painn_few_rows_limit()
    _compare(model, _batch(pos, z, ptr, model.cutoff_radius), tag="aspirin")


def test_water_box_192_with_virial_against_oracle():
    model = _model(3)
    pos, z, ptr, cell = syn.synth_water_box(4, seed=5)
    data = _batch(pos, z, ptr, model.cutoff_radius, cell=cell)
    deg = torch.bincount(data["edge_index"][0], minlength=len(z))
    assert int(deg.max()) > 16   # more than one staged chunk of edges per node
    with guard_bands.guard_allocations():
        _compare(model, data, virial=True, tag="water192")
        torch.cuda.synchronize()


def test_batch_with_single_atom_graphs_against_oracle():
    model = _model(4)
    pos, z, ptr = syn.synth_qm9_batch(4, seed=9)
    pos = np.concatenate([[[40.0, 0.0, 0.0]], pos, [[-40.0, 0.0, 0.0]]])
    z = np.concatenate([[1], z, [8]])
    ptr = np.concatenate([[0], ptr + 1, [len(z)]])
    got, _ = _compare(model, _batch(pos, z, ptr, model.cutoff_radius), tag="single_atoms")
    assert float(got["forces"][0].abs().max()) == 0.0 and float(got["forces"][-1].abs().max()) == 0.0


def test_one_hot_embedding_against_oracle():
    model = _model(5, embed_basis="one-hot")
    pos, z, ptr = syn.synth_qm9_batch(8, seed=11)
    _compare(model, _batch(pos, z, ptr, model.cutoff_radius), tag="one_hot")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 257, 2049])
def test_tile_edges(n):
    """Node counts around the 16-node tiles, the 4-node message workgroups and the few-row limit (2048); the last atom sits alone
    (degree 0)."""
    assert 2049 == lib.load().xeq_painn_few_rows_limit() + 1
    model = _model(6)
    rng = np.random.default_rng(n)
    side = max(2.0, (n / 0.05) ** (1.0 / 3.0))
    pos = rng.uniform(0, side, size=(n, 3))
    if n > 1:
        pos[-1] = [side + 20.0, 0.0, 0.0]
    z = rng.choice([1, 6, 7, 8], size=n)
    with guard_bands.guard_allocations():
        got, _ = _compare(model, _batch(pos, z, np.array([0, n]), model.cutoff_radius), tag=f"tile_edges_{n}")
        torch.cuda.synchronize()
    assert float(got["forces"][-1].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- bit stability
def test_repeats_shards_and_single_molecules_are_bitwise_equal():
    from xequinet_amd import dist

    model = _model(7)
    pos, z, ptr = syn.synth_qm9_batch(64, seed=5)
    whole = _eval(model, _batch(pos, z, ptr, model.cutoff_radius))
    again = _eval(model, _batch(pos, z, ptr, model.cutoff_radius))
    assert torch.equal(whole["energy"], again["energy"]) and torch.equal(whole["forces"], again["forces"])
    for world in (2, 4):
        Es, Fs = [], []
        for g0, g1 in dist.shard_by_edges(ptr, world):
            p_s, z_s, ptr_s = dist.take_shard(pos, z, ptr, g0, g1)
            part = _eval(model, _batch(p_s, z_s, ptr_s, model.cutoff_radius))
            Es.append(part["energy"]), Fs.append(part["forces"])
        assert torch.equal(torch.cat(Es), whole["energy"]) and torch.equal(torch.cat(Fs), whole["forces"]), world
    for g in (0, 5, 63):
        a0, a1 = int(ptr[g]), int(ptr[g + 1])
        one = _eval(model, _batch(pos[a0:a1], z[a0:a1], np.array([0, a1 - a0]), model.cutoff_radius))
        assert torch.equal(one["energy"], whole["energy"][g:g + 1]) and torch.equal(one["forces"], whole["forces"][a0:a1]), g


def test_launch_trace_holds_only_library_kernels():
    model = _model(8)
    pos, z, ptr = syn.synth_qm9_batch(8, seed=2)
    from xequinet_amd.nn.basic import edge_graph

    data = _batch(pos, z, ptr, model.cutoff_radius)
    edge_graph(data).n_rowptr   # the sorted views of the neighbour list are built once per list, outside the count
    _eval(model, data)   # packed weights
    first = lib.launch_count()
    _eval(model, data)
    names = lib.launch_names(first)
    print(names)
    assert all(n.startswith("xeq_") for n in names)
    assert sum(n.startswith("xeq_painn_") for n in names) == 3 * (1 + 2) + 3 * (1 + 2) + 2   # message fwd / bwd, update uv + out both ways, two adds
    assert len(names) == LAUNCHES_PER_EVALUATION, len(names)


# ----------------------------------------------------------------------------------------------------------------------- fronts
def test_graphed_model_replay_equals_eager():
    from xequinet_amd.runtime import GraphedModel

    model = _model(9)
    pos, z, ptr = syn.synth_qm9_batch(8, seed=4)
    data = _batch(pos, z, ptr, model.cutoff_radius)
    graphed = GraphedModel(model)
    for shift in (0.0, 0.05):   # the second geometry changes the edge list
        rng = np.random.default_rng(1)
        d = _batch(pos + shift * rng.standard_normal(pos.shape), z, ptr, model.cutoff_radius)
        eager = _eval(model, d)
        out = graphed(dict(d))
        assert torch.equal(out["energy"].detach(), eager["energy"]) and torch.equal(out["forces"].detach(), eager["forces"]), shift
    assert data is not None


@pytest.fixture
def model_units():
    """The default units a checkpoint's config carries (default_units); the process-wide map is put back afterwards."""
    from xequinet_amd.utils import units as U

    saved = dict(U.DEFAULT_UNITS_MAP)
    U.set_default_units({"energy": "eV"})
    yield
    U.DEFAULT_UNITS_MAP.clear()
    U.DEFAULT_UNITS_MAP.update(saved)


def test_ase_calculator_returns_the_models_energy_and_forces(model_units):
    from tests.test_gpu_interface import _Atoms
    from xequinet_amd.interface import XequiCalculator
    from xequinet_amd.interface.ase_calculator import _HAVE_ASE
    from xequinet_amd.utils import get_default_units, unit_conversion

    model = _model(11)
    pos, z, ptr = syn.synth_aspirin()
    if _HAVE_ASE:
        import ase

        atoms = ase.Atoms(numbers=z, positions=pos)
    else:   # the slice of ase.Atoms the calculator reads
        atoms = _Atoms(pos, z)
    want = _eval(model, _batch(pos, z, ptr, model.cutoff_radius))
    units = get_default_units()
    calc = XequiCalculator(model=model, tune_gemms=False)
    calc.calculate(atoms, ["energy", "forces"])
    e_fac, f_fac = unit_conversion(units[keys.TOTAL_ENERGY], "eV"), unit_conversion(units[keys.FORCES], "eV/Angstrom")
    np.testing.assert_allclose(calc.results["energy"], want["energy"].item() * e_fac, rtol=1e-6)
    np.testing.assert_allclose(calc.results["forces"], want["forces"].cpu().numpy() * f_fac, rtol=0, atol=1e-6)


def _front(mode, eager, **kw):
    from xequinet_amd.interface import resolve_jit_model

    front = resolve_jit_model(mode, model_name="painn", tune_gemms=False, **kw).to(DEV).eval().requires_grad_(False)
    front.load_state_dict(eager.state_dict())
    return front


@pytest.mark.parametrize("replay", [False, True])
def test_lammps_front_returns_the_eager_models_numbers_in_lammps_units(model_units, replay):
    """PaiNNLMP in LAMMPS "real" units (kcal/mol, Angstrom) on the periodic water box: the eager model's kernels on the same list, so
    energy, forces and virial are the eager model's bits times the unit factors."""
    from xequinet_amd.interface import PaiNNLMP
    from xequinet_amd.utils import unit_conversion

    eager = _model(12)
    pos, z, ptr, cell = syn.synth_water_box(4, seed=5)
    data = _batch(pos, z, ptr, eager.cutoff_radius, cell=cell)
    want = _eval(eager, data, virial=True)
    front = _front("lmp", eager, unit_style="real", replay=replay)
    assert isinstance(front, PaiNNLMP) and front.cutoff_radius == eager.cutoff_radius
    e_fac = unit_conversion("eV", "kcal/mol")
    assert front.energy_unit_factor == e_fac and front.forces_unit_factor == unit_conversion("eV/Angstrom", "kcal/mol/Angstrom")
    for _ in range(2):   # (the second call replays)
        lmp_data = {k: v for k, v in data.items() if k not in ("batch", "ptr")}   # LAMMPS hands over one graph, no batch
        got = front(lmp_data, True, True)
        assert torch.equal(got["energy"].detach(), want["energy"] * e_fac)
        assert torch.equal(got["forces"].detach(), want["forces"] * front.forces_unit_factor)
        assert torch.equal(got["virial"].detach(), want["virial"] * e_fac)
    with pytest.raises(NotImplementedError, match="PaiNN"):
        _front("lmp", eager, native=True)


@pytest.mark.parametrize("replay", [False, True])
def test_gromacs_front_searches_and_returns_the_eager_models_energy_and_forces(model_units, replay):
    """PaiNNGMX: positions in nm, energy in kJ/mol, forces from the caller's backward.  Its own neighbour search orders the list its
    own way, so the comparison is the project's f32 rule in model units (energy 1e-5 max|E| + 1e-4, forces 1e-4) times the unit
    factors, not bit equality."""
    from xequinet_amd.interface import PaiNNGMX
    from xequinet_amd.utils import unit_conversion

    eager = _model(13)
    pos, z, ptr = syn.synth_aspirin()
    want = _eval(eager, _batch(pos, z, ptr, eager.cutoff_radius))
    front = _front("gmx", eager, replay=replay)
    assert isinstance(front, PaiNNGMX)
    e_fac, f_fac = unit_conversion("eV", "kJ/mol"), unit_conversion("eV/Angstrom", "kJ/(mol*nm)")
    p_nm = (torch.tensor(pos, dtype=torch.float32, device=DEV) * unit_conversion("Angstrom", "nm")).requires_grad_()
    energy = front(p_nm, torch.tensor(z, device=DEV))
    (grad,) = torch.autograd.grad(energy.sum(), p_nm)
    de = float((energy.detach() - want["energy"] * e_fac).abs().max())
    df = float((-grad - want["forces"] * f_fac).abs().max())
    print({"gmx dE": de, "gmx dF": df})
    assert de <= (1e-5 * float(want["energy"].abs().max()) + 1e-4) * e_fac
    assert df <= 1e-4 * f_fac
    with pytest.raises(NotImplementedError, match="PaiNN"):
        _front("gmx", eager, whole_step=True)


def test_refusals_say_so():
    from xequinet_amd import runtime
    from xequinet_amd.interface.scripted import XPaiNNNative, compile_model

    model = _model(10)
    with pytest.raises(NotImplementedError, match="PaiNN"):
        XPaiNNNative(model)
    with pytest.raises(NotImplementedError, match="PaiNN"):
        compile_model(model, mode="lmp")
    with pytest.raises(NotImplementedError, match="PaiNN"):
        runtime.GraphedStep(model, torch.zeros((4, 3), device=DEV), torch.ones(4, dtype=torch.long, device=DEV))


# --------------------------------------------------------------------------------------------------------------------- training
def test_train_step_with_a_force_loss_moves_the_weights_and_the_packs_follow():
    """train.train_step on a small f32 batch (the tensor form in f32) with an energy + force loss: a finite loss, a gradient for every
    parameter, moved weights; the eval() evaluation behind it matches the oracle on the UPDATED state dict, i.e. the packed weight
    copies of the evaluation in front of the step were rebuilt."""
    from xequinet_amd.nn import training
    from xequinet_amd.train import train_step

    torch.manual_seed(3)
    model = resolve_model("painn").to(DEV)
    pos, z, ptr = syn.synth_qm9_batch(3, seed=6)
    data = _batch(pos, z, ptr, model.cutoff_radius)
    model.eval()
    training._warned_eval_params = False   # (said once per process)
    with pytest.warns(UserWarning, match="eval mode"):   # an eval-mode evaluation fills no parameter gradients, and says so
        before = _eval(model, data)   # packs the weights
    old = {k: v.detach().clone() for k, v in model.named_parameters()}
    target = {"energy": torch.zeros(len(ptr) - 1, device=DEV), "forces": torch.zeros((len(z), 3), device=DEV)}
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    loss, result = train_step(model, data, target, opt, {"energy": 1.0, "forces": 10.0})
    assert model.training and torch.isfinite(loss) and float(loss) > 0.0
    assert set(result) >= {"energy", "forces"} and not result["forces"].requires_grad
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
    moved = [k for k, p in model.named_parameters() if not torch.equal(p.detach(), old[k])]
    assert any(k.startswith("mods.message_0.rbf_lin") for k in moved) and any(k.startswith("mods.update_2.update_U") for k in moved), moved
    model.eval()
    after, ref = _compare(model, data, tag="after_train_step")
    bound = 1e-5 * float(ref["energy"].abs().max()) + 1e-4
    assert float((after["energy"] - before["energy"]).abs().max()) > 10 * bound   # the step was large enough to tell old packs from new


def test_f64_parameter_gradients_of_a_force_loss_against_oracle_autograd():
    """f64 is the tensor form itself: parameter gradients of an energy + force loss against oracle autograd to 1e-8."""
    torch.manual_seed(0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        model = resolve_model("painn").to(DEV).train()
    finally:
        torch.set_default_dtype(old)
    pos, z, ptr = syn.synth_qm9_batch(3, seed=6)
    data = _batch(pos, z, ptr, model.cutoff_radius)
    data["pos"] = data["pos"].double()
    out = model(dict(data), compute_forces=True)
    loss = out["energy"].sum() + (out["forces"] ** 2).sum()
    names = [k for k, _ in model.named_parameters() if "rbf.freq" not in k]
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(loss, [params[k] for k in names])
    q = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    c = lambda k: data[k].detach().cpu()
    ref = po.model(q, c("atomic_numbers").long(), c("pos"), c("edge_index"), c("batch").long(), len(ptr) - 1, 3, 5.0, create_graph=True)
    ref_grads = torch.autograd.grad(ref["energy"].sum() + (ref["forces"] ** 2).sum(), [q[k] for k in names])
    for k, g, r in zip(names, grads, ref_grads):
        assert float((g.cpu() - r).abs().max()) <= 1e-8 * max(1.0, float(r.abs().max())), k
