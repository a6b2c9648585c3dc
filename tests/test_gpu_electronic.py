"""GPU checks of the charge / spin embeddings (nn/electronic.py, csrc/xeq_electronic.hip): the kernels against the reference's own
outputs (tests/golden/electronic_f64.npz), the model against an f64 oracle that applies the restated modules after the embedding,
bit-stability (shards, batches, repeats), the MD fronts, the training pass and the refusals of the whole-step capture classes."""
import os

import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests.electronic_oracle import electronic, sub_params
from xequinet_amd import keys, lib
from xequinet_amd.data import NeighborTransform, XequiBatch
from xequinet_amd.data import synthetic as syn
from xequinet_amd.nn import resolve_model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
PARAMS = ("linear_q.weight", "linear_q.bias", "linear_k.weight", "linear_v.weight", "residual.mlp.0.weight", "residual.mlp.2.weight")


class ElectronicOracle(orc.XPaiNNOracle):
    """XPaiNNOracle with the restated charge / spin embeddings applied after ``embedding`` (nn/model.py:85-96)."""

    def embedding(self, data):
        data = super().embedding(data)
        for key, kind in ((keys.TOTAL_CHARGE, "charge"), (keys.TOTAL_SPIN, "spin")):
            prefix = f"mods.{kind}_embedding."
            if key in data and any(k.startswith(prefix) for k in self.sd):
                data["node_invariant"] = electronic(data["node_invariant"], data["batch"], data[key], sub_params(self.sd, prefix), kind)
        return data


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    model = resolve_model("xpainn", charge_embed=True, spin_embed=True, **kw)
    with torch.no_grad():   # weights that make the modules matter (the default init keeps them small)
        for name in ("charge_embedding", "spin_embedding"):
            for p in model.mods[name].parameters():
                p.mul_(3.0)
    return model


def _batch(pos, z, ptr, cutoff, charge=None, spin=None):
    b = XequiBatch(torch.tensor(pos, dtype=torch.float32), torch.tensor(z), torch.tensor(ptr),
                   charge=None if charge is None else torch.tensor(charge), spin=None if spin is None else torch.tensor(spin))
    b = b.to(DEV)
    return NeighborTransform(cutoff)(b)


def _eval(model, data, virial=False):
    with torch.enable_grad():
        out = model(dict(data), compute_forces=True, compute_virial=virial)
    return {k: v.detach() for k, v in out.items()}


def _host(d):
    keep = ("pos", "atomic_numbers", "edge_index", "batch", "ptr", "cell", "cell_offsets", "charge", "spin")
    out = {k: d[k].detach().cpu() for k in keep if k in d and isinstance(d[k], torch.Tensor)}
    out["pos"] = out["pos"].double()
    out["atomic_numbers"] = out["atomic_numbers"].long()
    if "cell" in out:
        out["cell"] = out["cell"].double()
        out["cell_offsets"] = out["cell_offsets"].double()
    return out


def _compare(model, data, virial=False):
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    sd32 = {k: v.float() for k, v in sd.items()}
    got = _eval(model, data, virial)
    host = _host(data)
    ref = ElectronicOracle(sd)(host, True, virial)
    ref32 = ElectronicOracle(sd32)({k: (v.float() if v.is_floating_point() else v) for k, v in host.items()}, True, virial)
    e, e_ref = got["energy"].cpu().double(), ref["energy"]
    assert float((e - e_ref).abs().max()) <= float(1e-5 * e_ref.abs().max() + 1e-4), (e, e_ref)
    err32 = float((ref32["forces"].double() - ref["forces"]).abs().max())
    df = float((got["forces"].cpu().double() - ref["forces"]).abs().max())
    assert df <= max(1e-4, 1.5 * err32), (df, err32)
    if virial:
        verr32 = float((ref32["virial"].double() - ref["virial"]).abs().max())
        dv = float((got["virial"].cpu().double() - ref["virial"]).abs().max())
        assert dv <= max(1e-4 * max(1.0, float(ref["virial"].abs().max())), 1.5 * verr32), (dv, verr32)
    return got, ref


# ----------------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("case", ["charge", "spin", "both"])
def test_kernel_against_reference_fixture(case):
    from xequinet_amd.nn.electronic import ChargeEmbedding, SpinEmbedding

    g = np.load(os.path.join(GOLDEN, "electronic_f64.npz"))
    F = int(g["node_dim"])
    assert lib.load().xeq_electronic_supported(lib.XEQ_F32, F)
    mods = []
    if case in ("charge", "both"):
        m = ChargeEmbedding(node_dim=F)
        m.load_state_dict({k: torch.tensor(g[f"w_c_{k}"]).float() for k in PARAMS})
        mods.append(m.to(DEV).eval().requires_grad_(False))
    if case in ("spin", "both"):
        m = SpinEmbedding(node_dim=F)
        m.load_state_dict({k: torch.tensor(g[f"w_s_{k}"]).float() for k in PARAMS})
        mods.append(m.to(DEV).eval().requires_grad_(False))
    s = torch.tensor(g["s"], dtype=torch.float32, device=DEV)
    data = {keys.NODE_INVARIANT: s, keys.BATCH: torch.tensor(g["batch"], device=DEV), keys.BATCH_PTR: torch.tensor(g["ptr"], device=DEV),
            keys.TOTAL_CHARGE: torch.tensor(g["charge"], device=DEV), keys.TOTAL_SPIN: torch.tensor(g["spin"], device=DEV)}
    n0 = lib.launch_count()
    for m in mods:
        data = m(data)
    torch.cuda.synchronize()
    assert lib.launch_names(n0).count("xeq_electronic_attn") == len(mods)
    assert lib.launch_names(n0).count("xeq_electronic_mix") == len(mods)
    ref = g[f"out_{case}"]
    got = data[keys.NODE_INVARIANT].cpu().double().numpy()
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max(), np.abs(got - ref).max()
    # graphs of 1 and 100 atoms (the 100-atom graph spans four tiles) are in the fixture
    assert 1 in np.diff(g["ptr"]) and np.diff(g["ptr"]).max() >= 100


@pytest.mark.parametrize("node_dim", [256, 128])
def test_kernel_at_full_width_against_restatement(node_dim):
    """The widest node_dim the kernels take (256: dynamic LDS above the default limit) and the default one, charge then spin on a
    batch with a one-atom graph and a graph over several tiles, f32 kernels against the f64 restatement."""
    from xequinet_amd.nn.electronic import ChargeEmbedding, SpinEmbedding

    torch.manual_seed(node_dim)
    mods = [ChargeEmbedding(node_dim=node_dim), SpinEmbedding(node_dim=node_dim)]
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                p.mul_(3.0)
    ptr = np.array([0, 1, 71, 72, 300, 333], dtype=np.int64)
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    charge, spin = np.array([2, -1, 0, -3, 1]), np.array([1, 0, 2, 4, 0])
    s64 = torch.randn(int(ptr[-1]), node_dim, dtype=torch.float64)
    want = s64
    for m, kind, t in zip(mods, ("charge", "spin"), (charge, spin)):
        want = electronic(want, torch.tensor(batch), torch.tensor(t), {k: v.double() for k, v in m.state_dict().items()}, kind)
    data = {keys.NODE_INVARIANT: s64.float().to(DEV), keys.BATCH: torch.tensor(batch, device=DEV), keys.BATCH_PTR: torch.tensor(ptr, device=DEV),
            keys.TOTAL_CHARGE: torch.tensor(charge, device=DEV), keys.TOTAL_SPIN: torch.tensor(spin, device=DEV)}
    n0 = lib.launch_count()
    for m in mods:
        data = m.to(DEV).eval().requires_grad_(False)(data)
    torch.cuda.synchronize()
    assert lib.launch_names(n0).count("xeq_electronic_mix") == 2
    got = data[keys.NODE_INVARIANT].cpu().double()
    assert float((got - want).abs().max()) <= 2e-6 * float(want.abs().max())


def test_kernel_entry_validates_arguments():
    from xequinet_amd import lib as L

    h = L.load()
    assert not h.xeq_electronic_supported(L.XEQ_F32, 48) and not h.xeq_electronic_supported(L.XEQ_F64, 128)
    st = h.xeq_electronic_fwd(2, None, 128, 0, 128, None, 1, None, None, None, None, None, None, None, None, None)
    assert st != 0 and b"kind" in h.xeq_last_error()


# ------------------------------------------------------------------------------------------------------------- model vs oracle
def test_aspirin_charged_radical_against_oracle():
    model = _model().to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_aspirin()
    data = _batch(pos, z, ptr, model.cutoff_radius, charge=[1], spin=[1]).to_dict()
    _compare(model, data)


def test_qm9_batch_mixed_charges_against_oracle():
    model = _model(1).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(64, seed=3)
    rng = np.random.default_rng(0)
    charge = rng.integers(-2, 3, size=64)
    spin = rng.integers(0, 3, size=64)
    _compare(model, _batch(pos, z, ptr, model.cutoff_radius, charge=charge, spin=spin).to_dict())


def test_water_box_charged_against_oracle():
    model = _model(2).to(DEV).eval().requires_grad_(False)
    f = np.load(os.path.join(GOLDEN, "radius_graph_pbc_water192.npz"))
    _, z, ptr, _ = syn.synth_water_box(4, seed=5)
    t = lambda a, dt=None: torch.tensor(a, device=DEV, dtype=dt)
    data = {"pos": t(f["pos"], torch.float32), "atomic_numbers": t(z.astype(np.int32)), "edge_index": t(f["edge_index"]),
            "ptr": t(ptr), "batch": t(np.zeros(len(z), dtype=np.int64)), "cell": t(f["cell"], torch.float32),
            "cell_offsets": t(f["cell_offsets"], torch.float32), "charge": t([-1]), "spin": t([2])}
    _compare(model, data, virial=True)


def test_charge_changes_the_result():
    model = _model().to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_aspirin()
    a = _eval(model, _batch(pos, z, ptr, model.cutoff_radius, charge=[0]).to_dict())
    b = _eval(model, _batch(pos, z, ptr, model.cutoff_radius, charge=[1]).to_dict())
    assert float((a["energy"] - b["energy"]).abs().max()) > 1e-4
    assert float((a["forces"] - b["forces"]).abs().max()) > 1e-5


def test_absent_keys_are_bit_identical_to_the_plain_model():
    model = _model().to(DEV).eval().requires_grad_(False)
    plain = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    plain.load_state_dict({k: v for k, v in model.state_dict().items() if "charge_embedding" not in k and "spin_embedding" not in k})
    pos, z, ptr = syn.synth_qm9_batch(16, seed=7)
    d = _batch(pos, z, ptr, model.cutoff_radius).to_dict()
    a, b = _eval(model, d), _eval(plain, d)
    assert torch.equal(a["energy"], b["energy"]) and torch.equal(a["forces"], b["forces"])


# ------------------------------------------------------------------------------------------------------------- bit-stability
def test_charged_batch_equals_its_shards_and_repeats():
    """A charged 256-molecule batch (the size of test_gpu_fullsize.py::test_sharded_equals_unsharded: every shard on the batch's side of
    the node-block threshold) equals its shards bit for bit -- dist.shard_by_edges / take_shard, charges and spins sliced to match --
    a molecule evaluated alone equals the same molecule inside a batch at the modules' output, and two evaluations repeat bit for bit."""
    from xequinet_amd import dist

    model = _model(3).to(DEV).eval().requires_grad_(False)
    seen = []
    model.mods["spin_embedding"].register_forward_hook(lambda mod, inp, out: seen.append(out[keys.NODE_INVARIANT].detach().clone()))
    pos, z, ptr = syn.synth_qm9_batch(256, seed=5)
    rng = np.random.default_rng(1)
    charge, spin = rng.integers(-2, 3, size=256), rng.integers(0, 3, size=256)
    whole = _eval(model, _batch(pos, z, ptr, model.cutoff_radius, charge=charge, spin=spin).to_dict())
    again = _eval(model, _batch(pos, z, ptr, model.cutoff_radius, charge=charge, spin=spin).to_dict())
    assert torch.equal(whole["energy"], again["energy"]) and torch.equal(whole["forces"], again["forces"])
    s_whole = seen[0]
    for world in (2, 4):
        Es, Fs = [], []
        for g0, g1 in dist.shard_by_edges(ptr, world):
            p_s, z_s, ptr_s = dist.take_shard(pos, z, ptr, g0, g1)
            part = _eval(model, _batch(p_s, z_s, ptr_s, model.cutoff_radius, charge=charge[g0:g1], spin=spin[g0:g1]).to_dict())
            Es.append(part["energy"]), Fs.append(part["forces"])
            assert torch.equal(seen[-1], s_whole[int(ptr[g0]):int(ptr[g1])])
        assert torch.equal(torch.cat(Es), whole["energy"]) and torch.equal(torch.cat(Fs), whole["forces"]), world
    g = 5   # one molecule alone: the modules' output equals the same molecule's rows inside the batch
    a0, a1 = int(ptr[g]), int(ptr[g + 1])
    _eval(model, _batch(pos[a0:a1], z[a0:a1], np.array([0, a1 - a0]), model.cutoff_radius, charge=charge[g:g + 1], spin=spin[g:g + 1]).to_dict())
    assert torch.equal(seen[-1], s_whole[a0:a1])


# --------------------------------------------------------------------------------------------------------------------- fronts
@pytest.fixture
def model_units():
    from xequinet_amd.utils import units as U

    saved = dict(U.DEFAULT_UNITS_MAP)
    U.set_default_units({"energy": "eV"})   # what a checkpoint's config carries (default_units)
    yield
    U.DEFAULT_UNITS_MAP.clear()
    U.DEFAULT_UNITS_MAP.update(saved)


def test_lammps_front_net_charge_eager_and_replay(model_units):
    from xequinet_amd.interface.md_model import XPaiNNLMP

    torch.manual_seed(0)
    kw = dict(charge_embed=True, spin_embed=False)
    eager = XPaiNNLMP(net_charge=1, **kw)
    with torch.no_grad():
        for p in eager.mods["charge_embedding"].parameters():
            p.mul_(3.0)
    eager = eager.to(DEV).eval().requires_grad_(False)
    replay = XPaiNNLMP(net_charge=1, replay=True, **kw).to(DEV).eval().requires_grad_(False)
    replay.load_state_dict(eager.state_dict())
    neutral = XPaiNNLMP(**kw).to(DEV).eval().requires_grad_(False)
    neutral.load_state_dict(eager.state_dict())
    pos, z, ptr = syn.synth_aspirin()
    ei = torch.tensor(orc.radius_graph_canonical(pos.astype(np.float32), ptr, eager.cutoff_radius), device=DEV)
    data = {"pos": torch.tensor(pos, dtype=torch.float32, device=DEV), "atomic_numbers": torch.tensor(z, device=DEV), "edge_index": ei}
    a = _eval(eager, data)
    for _ in range(2):
        b = _eval(replay, data)
    c = _eval(neutral, data)
    scale = float(a["forces"].abs().max())
    assert float((a["energy"] - b["energy"]).abs().max()) <= 1e-6 * max(1.0, float(a["energy"].abs().max()))
    assert float((a["forces"] - b["forces"]).abs().max()) <= 1e-6 * scale
    assert float((a["energy"] - c["energy"]).abs().max()) > 1e-4
    native = XPaiNNLMP(net_charge=1, native=True, **kw).to(DEV).eval().requires_grad_(False)
    native.load_state_dict(eager.state_dict())
    d = _eval(native, data)   # xeq::xpainn_eval with the charge embedding: the eager bits
    assert torch.equal(d["energy"], a["energy"]) and torch.equal(d["forces"], a["forces"])


def test_native_operator_equals_python_modules_for_a_charged_model():
    """xeq::xpainn_eval runs the charge / spin launches between the embedding and the first block: the same entry points in the
    same order as the Python modules, and the same bits; with no charge / spin handed over, the neutral model's bits."""
    from xequinet_amd import ops
    from xequinet_amd.interface.scripted import XPaiNNNative

    model = _model(5).to(DEV).eval().requires_grad_(False)
    native = XPaiNNNative(model)
    pos, z, ptr = syn.synth_qm9_batch(24, seed=13)
    rng = np.random.default_rng(2)
    charge, spin = torch.tensor(rng.integers(-2, 3, 24), device=DEV), torch.tensor(rng.integers(0, 3, 24), device=DEV)
    data = _batch(pos, z, ptr, model.cutoff_radius).to_dict()

    def py(with_el=True):
        d = dict(data)
        d[keys.EDGE_GRAPH] = ops.EdgeGraph(data["edge_index"], data["pos"].shape[0], center_sorted=True, ptr=data["ptr"], symmetric=True)
        if with_el:
            d["charge"], d["spin"] = charge, spin
        return _eval(model, d)

    def cc(with_el=True):
        return native(data["pos"].detach(), data["atomic_numbers"], data["edge_index"], data["ptr"], None, None, True, True, True, False,
                      charge if with_el else None, spin if with_el else None)

    py(), cc()   # packed weights, element tables: not part of a steady evaluation
    c0 = lib.launch_count()
    want = py()
    seq_py = lib.launch_names(c0)
    c0 = lib.launch_count()
    got = cc()
    seq_cc = lib.launch_names(c0)
    assert seq_py == seq_cc, "\n".join(f"{a:36s} {b}" for a, b in zip(seq_py + ["-"] * len(seq_cc), seq_cc + ["-"] * len(seq_py)) if a != b)
    assert seq_py.count("xeq_electronic_attn") == 2 and seq_py.count("xeq_electronic_mix") == 2
    assert "xeq_first_block_front" not in seq_py
    assert torch.equal(got[0], want["energy"]) and torch.equal(got[1], want["atomic_energies"]) and torch.equal(got[2], want["forces"])
    got0, want0 = cc(False), py(False)
    assert torch.equal(got0[0], want0["energy"]) and torch.equal(got0[2], want0["forces"])
    assert not torch.equal(got0[0], got[0])


def test_scripted_lammps_front_with_net_charge_saved_and_reloaded(tmp_path, model_units):
    """compile_model(..., net_charge=1): the scripted LAMMPS front, saved and reloaded, reproduces the eager XPaiNNLMP(net_charge=1)
    bit for bit, and differs from the neutral scripted front; the scripted GROMACS front with net_charge likewise."""
    from xequinet_amd.interface.md_model import XPaiNNGMX, XPaiNNLMP
    from xequinet_amd.interface.scripted import compile_model

    torch.manual_seed(0)
    lmp = XPaiNNLMP(net_charge=1, charge_embed=True)
    with torch.no_grad():
        for p in lmp.mods["charge_embedding"].parameters():
            p.mul_(3.0)
    lmp = lmp.to(DEV).eval().requires_grad_(False)
    path = str(tmp_path / "charged-lmp.jit")
    compile_model(lmp, mode="lmp", output_file=path, net_charge=1)
    loaded = torch.jit.load(path)
    neutral = compile_model(lmp, mode="lmp")
    pos, z, ptr = syn.synth_aspirin()
    b = _batch(pos, z, ptr, lmp.cutoff_radius)
    data = {"pos": b.pos, "atomic_numbers": b.atomic_numbers, "edge_index": b.edge_index}
    want = _eval(lmp, data)
    got = loaded(dict(data), True, False)
    assert torch.equal(got["energy"], want["energy"]) and torch.equal(got["forces"], want["forces"])
    assert float((neutral(dict(data), True, False)["energy"] - got["energy"]).abs().max()) > 1e-4

    gmx = XPaiNNGMX(net_charge=1, charge_embed=True).to(DEV).eval().requires_grad_(False)
    gmx.load_state_dict(lmp.state_dict())
    p_nm = (b.pos / 10.0).detach()
    e_eager = gmx(p_nm.clone().requires_grad_(), b.atomic_numbers)
    e_script = compile_model(gmx, mode="gmx", net_charge=1)(p_nm.clone(), b.atomic_numbers)
    e_neutral = compile_model(gmx, mode="gmx")(p_nm.clone(), b.atomic_numbers)
    assert torch.equal(e_script.detach(), e_eager.detach())
    assert float((e_script - e_neutral).abs().max()) > 1e-4


def test_gromacs_front_net_charge_matters(model_units):
    from xequinet_amd.interface.md_model import XPaiNNGMX

    torch.manual_seed(0)
    with_q = XPaiNNGMX(net_charge=1, charge_embed=True)
    with torch.no_grad():
        for p in with_q.mods["charge_embedding"].parameters():
            p.mul_(3.0)
    with_q = with_q.to(DEV).eval().requires_grad_(False)
    without = XPaiNNGMX(charge_embed=True).to(DEV).eval().requires_grad_(False)
    without.load_state_dict(with_q.state_dict())
    pos, z, _ = syn.synth_aspirin()
    e = []
    for m in (with_q, without):
        p = torch.tensor(pos, dtype=torch.float32, device=DEV) / 10.0   # nm
        out = m(p.requires_grad_(True), torch.tensor(z, device=DEV))
        e.append(float(out.detach().reshape(-1)[0]) if isinstance(out, torch.Tensor) else float(out[0].detach().reshape(-1)[0]))
    assert abs(e[0] - e[1]) > 1e-4


# ------------------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-8), (torch.float32, 2e-4)])
def test_training_gradients_of_the_electronic_parameters(dtype, tol):
    """model.train(), energy + force loss: the gradients of charge_embedding.* / spin_embedding.* against the f64 oracle's autograd.
    f64: 1e-8 of the largest entry.  f32: test_gpu_training.py's 2e-4 of the largest entry, widened only to 1.5 x what fp32 rounding
    does to the reference's own arithmetic on the same inputs (the oracle with fp32 weights against the fp64 one, as in
    test_gpu_parity.py's force bounds): a force loss's parameter gradients are a second derivative."""
    from xequinet_amd.nn import training

    torch.manual_seed(4)
    model = _model(4).to(dtype).to(DEV).train()
    assert not training.native_pass_supported(model)
    pos, z, ptr = syn.synth_qm9_batch(3, seed=21)
    ei = orc.radius_graph_canonical(pos, ptr, 5.0)
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    host = {"pos": torch.tensor(pos, dtype=torch.float64), "atomic_numbers": torch.tensor(z.astype(np.int64)), "edge_index": torch.tensor(ei),
            "batch": torch.tensor(batch), "ptr": torch.tensor(ptr), "charge": torch.tensor([1, -1, 0]), "spin": torch.tensor([1, 0, 2])}
    dev = {k: (v.to(dtype) if v.is_floating_point() else v).to(DEV) for k, v in host.items()}
    out = model(dict(dev), compute_forces=True, compute_virial=False)
    loss = (out["energy"] ** 2).sum() + (out["forces"] ** 2).sum()
    loss.backward()
    sd = {k: v.detach().cpu().double().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    ref = ElectronicOracle(sd)(host, True, False, training=True)
    ref_loss = (ref["energy"] ** 2).sum() + (ref["forces"] ** 2).sum()
    assert abs(loss.item() - ref_loss.item()) <= (1e-9 if dtype == torch.float64 else 1e-4) * max(1.0, abs(ref_loss.item()))
    names = [n for n, _ in model.named_parameters() if "charge_embedding" in n or "spin_embedding" in n]
    assert len(names) == 12
    grads = dict(zip(names, torch.autograd.grad(ref_loss, [sd[n] for n in names])))
    err32 = {n: 0.0 for n in names}
    if dtype == torch.float32:
        sd32 = {k: v.detach().float().clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        host32 = {k: (v.float() if v.is_floating_point() else v) for k, v in host.items()}
        r32 = ElectronicOracle(sd32)(host32, True, False, training=True)
        g32 = torch.autograd.grad((r32["energy"] ** 2).sum() + (r32["forces"] ** 2).sum(), [sd32[n] for n in names])
        err32 = {n: (g.double() - grads[n]).abs().max().item() for n, g in zip(names, g32)}
    params = dict(model.named_parameters())
    for n in names:
        g_ref = grads[n]
        err = (params[n].grad.double().cpu() - g_ref).abs().max().item()
        bound = max(tol * max(1e-6, g_ref.abs().max().item()), 1.5 * err32[n])
        assert err <= bound, f"{n}: {err:.2e} of {g_ref.abs().max().item():.2e} (fp32 oracle {err32[n]:.2e})"


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_whole_step_classes_refuse_a_charged_model():
    from xequinet_amd import runtime, train

    model = _model().to(DEV).eval()
    cap = (64, 2, 1024)
    with pytest.raises(ValueError, match="charge"):
        runtime.GraphedStep(model, cap)
    with pytest.raises(ValueError, match="charge"):
        runtime.GraphedLanes(model, cap)
    with pytest.raises(ValueError, match="charge"):
        runtime.GraphedStepsInFlight(model, cap)
    with pytest.raises(ValueError, match="charge"):
        runtime.GraphedChunks(model, [0, 21, 42])
    with pytest.raises(ValueError, match="charge"):
        runtime.GraphedStepPBC(model, 64, 1024)
    with pytest.raises(ValueError, match="charge"):
        train.GraphedTrainStep(model.train(), torch.optim.Adam(model.parameters()), cap)
