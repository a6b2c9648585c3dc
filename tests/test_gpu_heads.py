"""GPU checks of the property heads (nn/output.py: ScalarOut, AtomicChargesOut, PolarOut; csrc/xeq_heads.hip): the kernels against the
restatement of tests/heads_oracle.py with their launch budget and guard bands, whole models against the f64 oracle, equivariance on
the device, bit-stability (shards, batches, repeats), the unchanged default model, HIP-graph replay, the fronts' refusals and the
training pass.

Bound of every comparison with the f64 restatement: |got - ref64| <= max(2e-6 max|ref64|, 1.5 max|ref32 - ref64|), ref32 the same
restatement in f32 on the same inputs -- 2e-6 is a few f32 roundings of the largest entry, the second term what the number format
alone does to the reference's own arithmetic (the ||d|| term of the polarizability cancels for near-isotropic graphs, so a fixed
relative bound would be wrong there)."""
import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests import guard_bands
from tests import heads_oracle as ho
from xequinet_amd import keys, lib
from xequinet_amd.data import NeighborTransform, XequiBatch
from xequinet_amd.data import synthetic as syn
from xequinet_amd.nn import resolve_model, resolve_output

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = {
    "default": dict(node_dim=128, node_irreps="128x0e + 64x1o + 32x2e", hidden_dim=64, hidden_irreps="64x0e + 16x2e"),
    "narrow": dict(node_dim=32, node_irreps="32x0e+16x1o+8x2e", hidden_dim=16, hidden_irreps="16x0e+4x2e"),
}
HEADS = ("output_scalar", "output_charges", "output_polar")


def _close(got, ref64, ref32, what):
    got, ref32 = got.detach().cpu().double(), ref32.detach().double()
    err = float((got - ref64).abs().max())
    bound = max(2e-6 * float(ref64.abs().max()), 1.5 * float((ref32 - ref64).abs().max()))
    print(f"{what}: err {err:.3e} bound {bound:.3e} (max|ref| {float(ref64.abs().max()):.3e})")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _scaled(model, names=HEADS):
    with torch.no_grad():   # weights that make the heads matter
        for name in names:
            if name in model.mods:
                for p in model.mods[name].parameters():
                    p.mul_(3.0)
                    if p.dim() == 1 and float(p.abs().max()) == 0.0:
                        p.add_(0.1 * torch.randn_like(p))
    return model


def _batch(pos, z, ptr, cutoff, charge=None):
    b = XequiBatch(torch.tensor(pos, dtype=torch.float32), torch.tensor(z), torch.tensor(ptr), charge=None if charge is None else torch.tensor(charge))
    return NeighborTransform(cutoff)(b.to(DEV))


def _eval(model, data, forces=True):
    with torch.enable_grad():
        out = model(dict(data), compute_forces=forces, compute_virial=False)
    return {k: v.detach() for k, v in out.items()}


def _host(d, dtype=torch.float64):
    out = {k: d[k].detach().cpu() for k in ("pos", "atomic_numbers", "edge_index", "batch", "ptr", "charge") if k in d}
    out["pos"] = out["pos"].to(dtype)
    out["atomic_numbers"] = out["atomic_numbers"].long()
    return out


def _oracles(model, data, forces, **kw):
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    o64, o32 = ho.HeadsOracle(sd, **kw), ho.HeadsOracle({k: v.float() for k, v in sd.items()}, **kw)
    r64, r32 = o64(_host(data), forces, False), o32(_host(data, torch.float32), forces, False)
    r64.update({k: v.detach() for k, v in o64.heads.items()})
    r32.update({k: v.detach() for k, v in o32.heads.items()})
    return r64, r32


# ----------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", ["default", "narrow"])
def test_kernels_against_restatement_with_budget_and_guard_bands(case):
    kw = WIDTHS[case]
    torch.manual_seed(3)
    F, D = kw["node_dim"], orc.irreps_dim(kw["node_irreps"])
    ptr = np.array([0, 1, 3, 32, 132, 133], dtype=np.int64)   # graphs of 1, 2, 29, 100 and 1 atoms; N = 133 is no multiple of the tile
    N, G = int(ptr[-1]), len(ptr) - 1
    batch = torch.tensor(np.repeat(np.arange(G), np.diff(ptr)))
    charge = torch.tensor([1, -2, 0, 2, -1])
    heads = {"scalar": resolve_output("scalar", **kw), "mean": resolve_output("scalar", reduce_op="mean", **kw), "charges": resolve_output("charges", **kw),
             "polar": resolve_output("polar", isotropic=True, **kw)}
    with torch.no_grad():
        for h in heads.values():
            for p in h.parameters():
                p.mul_(3.0)
                if p.dim() == 1 and float(p.abs().max()) == 0.0:
                    p.add_(0.1 * torch.randn_like(p))
    s64, x64 = torch.randn(N, F, dtype=torch.float64), torch.randn(N, D, dtype=torch.float64)
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = {k: {n: v.detach().to(dt) for n, v in h.state_dict().items()} for k, h in heads.items()}
        s, x = s64.to(dt), x64.to(dt)
        alpha, iso = ho.polar_out(s, x, batch, G, p["polar"], kw["node_irreps"], kw["hidden_irreps"])
        ref[dt] = {"scalar": ho.scalar_out(s, batch, G, p["scalar"]), "mean": ho.scalar_out(s, batch, G, p["mean"], "mean"),
                   "charges": ho.charges_out(s, batch, G, p["charges"], charge), "alpha": alpha, "iso": iso,
                   "t": ho.polar_nodes(s, x, p["polar"], kw["node_irreps"], kw["hidden_irreps"])}
    for h in heads.values():
        h.to(DEV).eval().requires_grad_(False)
    xbig = torch.zeros(N, D + 8, dtype=torch.float32, device=DEV)
    xbig[:, 4:4 + D] = x64.float().to(DEV)
    x_view = xbig[:, 4:4 + D]                                   # a strided view, as the node block hands them out
    assert x_view.stride(0) == D + 8 and not x_view.is_contiguous()

    def data():
        return {keys.NODE_INVARIANT: s64.float().to(DEV), keys.NODE_EQUIVARIANT: x_view, keys.BATCH: batch.to(DEV),
                keys.BATCH_PTR: torch.tensor(ptr, device=DEV), keys.TOTAL_CHARGE: charge.to(DEV)}

    for h in heads.values():    # packed weights: not part of a steady evaluation
        h(data())
    with guard_bands.guard_allocations() as guards:
        out, names = {}, {}
        for k, h in heads.items():
            n0 = lib.launch_count()
            out[k] = h(data())
            names[k] = lib.launch_names(n0)
        torch.cuda.synchronize()
    assert guards.count >= 4      # t, alpha, iso and the head rows at least: every band is checked on leaving the block
    assert names["polar"] == ["xeq_head_polar_nodes", "xeq_head_graph_reduce"], names["polar"]
    if case == "default":         # the scalar and charge MLPs on the energy head's kernel + one reduction
        for k in ("scalar", "mean", "charges"):
            assert names[k] == ["xeq_head_fwd", "xeq_head_graph_reduce"], (k, names[k])
    r64, r32 = ref[torch.float64], ref[torch.float32]
    _close(out["scalar"][keys.SCALAR_OUTPUT], r64["scalar"], r32["scalar"], "scalar sum")
    _close(out["mean"][keys.SCALAR_OUTPUT], r64["mean"], r32["mean"], "scalar mean")
    _close(out["charges"][keys.ATOMIC_CHARGES], r64["charges"], r32["charges"], "charges")
    _close(out["polar"][keys.POLARIZABILITY], r64["alpha"], r32["alpha"], "alpha")
    _close(out["polar"][keys.ISO_POLARIZABILITY], r64["iso"], r32["iso"], "iso")
    assert out["polar"][keys.POLARIZABILITY].shape == (G, 3, 3) and out["charges"][keys.ATOMIC_CHARGES].shape == (N,)
    q = out["charges"][keys.ATOMIC_CHARGES].cpu().double()
    assert bool(((ho.graph_sum(q, batch, G) - charge.double()).abs() <= 1e-5 * torch.tensor(np.diff(ptr), dtype=torch.float64)).all())
    assert float(xbig[:, :4].abs().max()) == 0.0 and float(xbig[:, 4 + D:].abs().max()) == 0.0
    # the node pass alone: t [N, 8] with its pad written as zeros, nothing outside the extents
    polar = heads["polar"]
    mul0, mul2, off2, hid0, hid2 = polar._widths()
    ws1, w0, w2 = polar._packs()
    t = guard_bands.guarded((N, 8), torch.float32, DEV)
    s32 = s64.float().to(DEV)
    lib.call("xeq_head_polar_nodes", lib.ptr(s32), s32.stride(0), lib.ptr(x_view), x_view.stride(0), N, F, mul0, mul2, off2, kw["hidden_dim"], hid0, hid2,
             lib.ptr(ws1), lib.ptr(w0), lib.ptr(w2), lib.ptr(polar.scalar_out_mlp[2].weight), lib.ptr(polar.scalar_out_mlp[2].bias),
             lib.ptr(polar.equi_out_mlp[2].weight), lib.ptr(polar.equi_out_mlp[2].bias), 1e-5, lib.ptr(t), lib.stream())
    torch.cuda.synchronize()
    guard_bands.check(t)
    assert not bool(guard_bands.unwritten(t).any()) and float(t[:, 6:].abs().max()) == 0.0
    _close(t[:, :6], r64["t"], r32["t"], "t")


def test_empty_graph_gives_zeros():
    ptr = torch.tensor([0, 3, 3, 5], device=DEV)
    src = torch.arange(40, dtype=torch.float32, device=DEV).reshape(5, 8) + 1.0
    out = torch.full((3, 6), 7.0, device=DEV)
    for mode in (0, 1):
        lib.call("xeq_head_graph_reduce", mode, lib.ptr(src), 8, 6, lib.ptr(ptr), 3, None, lib.ptr(out), None, lib.stream())
        want = torch.stack([src[:3, :6].sum(0), torch.zeros(6, device=DEV), src[3:, :6].sum(0)])
        if mode == 1:
            want = want / torch.tensor([3.0, 1.0, 2.0], device=DEV)[:, None]
        assert torch.allclose(out, want, rtol=1e-6, atol=0) and float(out[1].abs().max()) == 0.0
    alpha, iso = torch.full((3, 9), 7.0, device=DEV), torch.full((3,), 7.0, device=DEV)
    lib.call("xeq_head_graph_reduce", 2, lib.ptr(src), 8, 6, lib.ptr(ptr), 3, None, lib.ptr(alpha), lib.ptr(iso), lib.stream())
    assert float(alpha[1].abs().max()) == 0.0 and float(iso[1]) == 0.0 and bool(torch.isfinite(alpha).all())
    q = src[:, 0].clone()
    lib.call("xeq_head_graph_reduce", 3, lib.ptr(q), 1, 1, lib.ptr(ptr), 3, None, None, None, lib.stream())
    assert bool(torch.isfinite(q).all()) and abs(float(q[:3].sum())) <= 1e-4 and abs(float(q[3:].sum())) <= 1e-4


# ------------------------------------------------------------------------------------------------------------- model vs oracle
def test_aspirin_energy_forces_and_polarizability_against_oracle():
    torch.manual_seed(0)
    model = _scaled(resolve_model("xpainn", output_modes=["energy", "polar"])).to(DEV).eval().requires_grad_(False)
    assert model.mods["update_2"].equivariant_output_unused is False
    pos, z, ptr = syn.synth_aspirin()
    data = _batch(pos, z, ptr, model.cutoff_radius).to_dict()
    got = _eval(model, data)
    r64, r32 = _oracles(model, data, True)
    e, e_ref = got["energy"].cpu().double(), r64["energy"]
    assert float((e - e_ref).abs().max()) <= float(1e-5 * e_ref.abs().max() + 1e-4)
    err32 = float((r32["forces"].double() - r64["forces"]).abs().max())
    assert float((got["forces"].cpu().double() - r64["forces"]).abs().max()) <= max(1e-4, 1.5 * err32)
    assert float(r64["polarizability"].abs().max()) > 1e-3
    _close(got["polarizability"], r64["polarizability"], r32["polarizability"], "aspirin alpha")
    assert "iso_polarizability" not in got


def test_qm9_scalar_and_charges_against_oracle():
    torch.manual_seed(1)
    model = _scaled(resolve_model("xpainn", output_modes=["scalar", "charges"])).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(16, seed=3)
    charge = np.random.default_rng(0).integers(-2, 3, size=16)
    data = _batch(pos, z, ptr, model.cutoff_radius, charge=charge).to_dict()
    with pytest.raises(KeyError, match="energy"):
        model(dict(data), compute_forces=True)
    got = _eval(model, data, forces=False)
    assert set(got) == {"scalar_output", "atomic_charges"}
    r64, r32 = _oracles(model, data, False)
    _close(got["scalar_output"], r64["scalar_output"], r32["scalar_output"], "qm9 scalar")
    _close(got["atomic_charges"], r64["atomic_charges"], r32["atomic_charges"], "qm9 charges")
    sums = ho.graph_sum(got["atomic_charges"].cpu().double(), data["batch"].cpu(), 16)
    assert bool(((sums - torch.tensor(charge, dtype=torch.float64)).abs() <= 1e-5 * torch.tensor(np.diff(ptr), dtype=torch.float64)).all())


def _rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_polarizability_rotates_as_a_tensor_on_the_device():
    torch.manual_seed(2)
    model = _scaled(resolve_model("xpainn", output_modes=["energy", "polar"])).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_aspirin()
    R = _rotation(7)
    d0, d1 = _batch(pos, z, ptr, model.cutoff_radius).to_dict(), _batch(pos @ R.T, z, ptr, model.cutoff_radius).to_dict()
    a0, a1 = _eval(model, d0)["polarizability"][0].cpu().double(), _eval(model, d1)["polarizability"][0].cpu().double()
    sd32 = {k: v.detach().cpu().float() for k, v in model.state_dict().items()}
    o = ho.HeadsOracle(sd32)
    o(_host(d0, torch.float32), False, False)
    b0 = o.heads["polarizability"][0].detach().double()
    o(_host(d1, torch.float32), False, False)
    b1 = o.heads["polarizability"][0].detach().double()
    Rt = torch.tensor(R)
    own = float((b1 - Rt @ b0 @ Rt.T).abs().max())     # what f32 does to the restatement's own equivariance
    err = float((a1 - Rt @ a0 @ Rt.T).abs().max())
    print(f"equivariance: device {err:.3e}, f32 oracle {own:.3e}, max|alpha| {float(a0.abs().max()):.3e}")
    assert err <= max(1.5 * own, 1e-5 * float(a0.abs().max()))


# ------------------------------------------------------------------------------------------------------------- bit-stability
def test_batch_equals_its_shards_a_lone_molecule_and_repeats():
    """A 256-molecule batch (every shard on the batch's side of the node-block threshold) equals its 2 and 4 shards bit for bit in every
    head's output, and repeats bit for bit.  One molecule alone: the heads, given that molecule's rows of the trunk's output, return the
    bits of its rows in the batch (as test_gpu_electronic.py checks its modules' output; the trunk picks its message kernels by size,
    so a whole-model evaluation of a lone molecule is compared only where the trunk handed the heads the same bits)."""
    from xequinet_amd import dist

    torch.manual_seed(3)
    model = _scaled(resolve_model("xpainn", output_modes=["energy", "polar", "charges", "scalar"])).to(DEV).eval().requires_grad_(False)
    seen = []
    model.mods["update_2"].register_forward_hook(
        lambda mod, inp, out: seen.append((out[keys.NODE_INVARIANT].detach().clone(), out[keys.NODE_EQUIVARIANT].detach().clone())))
    pos, z, ptr = syn.synth_qm9_batch(256, seed=5)
    charge = np.random.default_rng(1).integers(-2, 3, size=256)
    names = ("polarizability", "atomic_charges", "scalar_output", "energy", "forces")
    whole = _eval(model, _batch(pos, z, ptr, model.cutoff_radius, charge=charge).to_dict())
    s_whole, x_whole = seen[0]
    again = _eval(model, _batch(pos, z, ptr, model.cutoff_radius, charge=charge).to_dict())
    for k in names:
        assert torch.equal(whole[k], again[k]), k
    for world in (2, 4):
        parts = {k: [] for k in names}
        for g0, g1 in dist.shard_by_edges(ptr, world):
            p_s, z_s, ptr_s = dist.take_shard(pos, z, ptr, g0, g1)
            part = _eval(model, _batch(p_s, z_s, ptr_s, model.cutoff_radius, charge=charge[g0:g1]).to_dict())
            for k in names:
                parts[k].append(part[k])
        for k in names:
            assert torch.equal(torch.cat(parts[k]), whole[k]), (world, k)
    g = 5
    a0, a1 = int(ptr[g]), int(ptr[g + 1])
    rows = {keys.NODE_INVARIANT: s_whole[a0:a1], keys.NODE_EQUIVARIANT: x_whole[a0:a1], keys.BATCH: torch.zeros(a1 - a0, dtype=torch.long, device=DEV),
            keys.BATCH_PTR: torch.tensor([0, a1 - a0], device=DEV), keys.TOTAL_CHARGE: torch.tensor(charge[g:g + 1], device=DEV)}
    for name in HEADS:
        rows = model.mods[name](rows)
    assert torch.equal(rows["polarizability"][0], whole["polarizability"][g]) and torch.equal(rows["scalar_output"][0], whole["scalar_output"][g])
    assert torch.equal(rows["atomic_charges"], whole["atomic_charges"][a0:a1])
    one = _eval(model, _batch(pos[a0:a1], z[a0:a1], np.array([0, a1 - a0]), model.cutoff_radius, charge=charge[g:g + 1]).to_dict())
    trunk_same = torch.equal(seen[-1][0], s_whole[a0:a1]) and torch.equal(seen[-1][1], x_whole[a0:a1])
    print(f"lone molecule: trunk output bit-equal to its rows in the batch: {trunk_same}")
    if trunk_same:
        assert torch.equal(one["polarizability"][0], whole["polarizability"][g]) and torch.equal(one["atomic_charges"], whole["atomic_charges"][a0:a1])


def test_last_block_writes_x_on_both_sides_of_the_node_block_threshold():
    """The fused node block runs from a node count on (xeq_node_block_auto), the split kernels below it: with a polar head both must form
    the last block's equivariant output.  A batch above the threshold against its two shards below it."""
    from xequinet_amd import dist

    torch.manual_seed(4)
    model = _scaled(resolve_model("xpainn", output_modes=["energy", "polar"])).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(420, seed=9)
    auto = lib.load().xeq_node_block_auto
    shards = list(dist.shard_by_edges(ptr, 2))
    assert auto(int(ptr[-1])) and not any(auto(int(ptr[g1] - ptr[g0])) for g0, g1 in shards)
    n0 = lib.launch_count()
    whole = _eval(model, _batch(pos, z, ptr, model.cutoff_radius).to_dict())["polarizability"]
    assert "xeq_node_block_fwd" in lib.launch_names(n0)
    parts = []
    for g0, g1 in shards:
        p_s, z_s, ptr_s = dist.take_shard(pos, z, ptr, g0, g1)
        n0 = lib.launch_count()
        parts.append(_eval(model, _batch(p_s, z_s, ptr_s, model.cutoff_radius).to_dict())["polarizability"])
        assert "xeq_node_block_fwd" not in lib.launch_names(n0)
    parts = torch.cat(parts)
    assert float(whole.abs().max()) > 1e-3
    assert float((parts - whole).abs().max()) <= 1e-5 * float(whole.abs().max())


def test_default_model_is_unchanged_by_a_second_head():
    torch.manual_seed(5)
    plain = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    both = resolve_model("xpainn", output_modes=["energy", "scalar"]).to(DEV).eval().requires_grad_(False)
    both.load_state_dict({**both.state_dict(), **plain.state_dict()})
    pos, z, ptr = syn.synth_qm9_batch(16, seed=7)
    d = _batch(pos, z, ptr, plain.cutoff_radius).to_dict()
    _eval(plain, d), _eval(both, d)
    n0 = lib.launch_count()
    a = _eval(plain, d)
    seq_a = lib.launch_names(n0)
    n0 = lib.launch_count()
    b = _eval(both, d)
    seq_b = lib.launch_names(n0)
    assert torch.equal(a["energy"], b["energy"]) and torch.equal(a["forces"], b["forces"]) and torch.equal(a["atomic_energies"], b["atomic_energies"])
    extra = ["xeq_head_fwd", "xeq_head_graph_reduce"]
    assert "xeq_head_graph_reduce" not in seq_a and "xeq_head_polar_nodes" not in seq_a
    i = seq_b.index("xeq_head_graph_reduce")
    assert seq_b[i - 1:i + 1] == extra and seq_b[:i - 1] + seq_b[i + 1:] == seq_a, (seq_a, seq_b)


# ---------------------------------------------------------------------------------------------------------------------- fronts
def test_graphed_model_replays_a_polar_model_to_the_eager_bits():
    from xequinet_amd import runtime

    torch.manual_seed(6)
    model = _scaled(resolve_model("xpainn", output_modes=["energy", "polar", "charges"])).to(DEV).eval().requires_grad_(False)
    pos, z, ptr = syn.synth_qm9_batch(8, seed=11)
    d = _batch(pos, z, ptr, model.cutoff_radius, charge=np.array([1, 0, -1, 0, 2, 0, 0, -2])).to_dict()
    want = _eval(model, d)
    gm = runtime.GraphedModel(model, tune_gemms=False)
    for _ in range(2):
        got = {k: v.clone() for k, v in gm(dict(d)).items()}
    for k in ("energy", "forces", "polarizability", "atomic_charges"):
        assert torch.equal(got[k], want[k]), k


def test_energy_only_fronts_refuse_a_model_with_another_head():
    from xequinet_amd import runtime, train
    from xequinet_amd.interface.scripted import XPaiNNNative, compile_model

    model = resolve_model("xpainn", output_modes=["energy", "polar"]).to(DEV).eval()
    cap = (64, 2, 1024)
    for make in (lambda: runtime.GraphedStep(model, cap), lambda: runtime.GraphedLanes(model, cap), lambda: runtime.GraphedStepsInFlight(model, cap),
                 lambda: runtime.GraphedChunks(model, [0, 21, 42]), lambda: runtime.GraphedStepPBC(model, 64, 1024),
                 lambda: XPaiNNNative(model), lambda: compile_model(model, mode="lmp"),
                 lambda: train.GraphedTrainStep(model.train(), torch.optim.Adam(model.parameters()), cap)):
        with pytest.raises(ValueError, match="output head"):
            make()


# -------------------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-8), (torch.float32, 2e-4)])
def test_training_gradients_of_the_head_parameters(dtype, tol):
    """model.train(), loss (alpha^2).sum() + (q^2).sum(): every head parameter's gradient against the f64 oracle's autograd.  f64: 1e-8
    of the largest entry; f32: 2e-4 of it (test_gpu_training.py's bound), or 1.5 x what f32 does to the oracle's own gradient."""
    from xequinet_amd.nn import training

    torch.manual_seed(8)
    model = _scaled(resolve_model("xpainn", output_modes=["energy", "polar", "charges"])).to(dtype).to(DEV).train()
    assert not training.native_pass_supported(model)
    pos, z, ptr = syn.synth_qm9_batch(3, seed=21)
    ei = orc.radius_graph_canonical(pos, ptr, 5.0)
    host = {"pos": torch.tensor(pos, dtype=torch.float64), "atomic_numbers": torch.tensor(z.astype(np.int64)), "edge_index": torch.tensor(ei),
            "batch": torch.tensor(np.repeat(np.arange(3), np.diff(ptr))), "ptr": torch.tensor(ptr), "charge": torch.tensor([1, -1, 0])}
    dev = {k: (v.to(dtype) if v.is_floating_point() else v).to(DEV) for k, v in host.items()}
    out = model(dict(dev), compute_forces=False, compute_virial=False)
    loss = (out["polarizability"] ** 2).sum() + (out["atomic_charges"] ** 2).sum()
    loss.backward()
    names = [n for n, _ in model.named_parameters() if "output_polar" in n or "output_charges" in n]
    assert len(names) == 12

    def oracle_grads(dt):
        sd = {k: v.detach().cpu().to(dt).clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
        o = ho.HeadsOracle(sd)
        o({k: (v.to(dt) if v.is_floating_point() else v) for k, v in host.items()}, False, False, training=True)
        ref_loss = (o.heads["polarizability"] ** 2).sum() + (o.heads["atomic_charges"] ** 2).sum()
        return ref_loss, dict(zip(names, torch.autograd.grad(ref_loss, [sd[n] for n in names])))

    ref_loss, grads = oracle_grads(torch.float64)
    assert abs(loss.item() - ref_loss.item()) <= (1e-9 if dtype == torch.float64 else 1e-4) * max(1.0, abs(ref_loss.item()))
    err32 = {n: 0.0 for n in names}
    if dtype == torch.float32:
        _, g32 = oracle_grads(torch.float32)
        err32 = {n: (g32[n].double() - grads[n]).abs().max().item() for n in names}
    params = dict(model.named_parameters())
    for n in names:
        g_ref = grads[n]
        err = (params[n].grad.double().cpu() - g_ref).abs().max().item()
        bound = max(tol * max(1e-6, g_ref.abs().max().item()), 1.5 * err32[n])
        print(f"{n}: err {err:.2e} bound {bound:.2e}")
        assert err <= bound, f"{n}: {err:.2e} of {g_ref.abs().max().item():.2e} (fp32 oracle {err32[n]:.2e})"
