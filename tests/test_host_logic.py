"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol that
include/xeq.h declares, host-side mirrors keep the reference's interface, and the
product refuses to run without HIP tensors (no CPU fallback)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from xequinet_amd import lib

    header = open(os.path.join(ROOT, "include", "xeq.h")).read()
    declared = set(re.findall(r"\b(xeq_[a-z0-9_]+)\s*\(", header))
    assert declared, "no prototypes parsed"
    handle = lib.load()
    for name in sorted(declared):
        assert hasattr(handle, name), f"{name} declared in xeq.h but not exported"
    assert declared == set(lib.EXPORTS), declared ^ set(lib.EXPORTS)
    assert handle.xeq_version() >= 100


def test_c_abi_argument_errors_are_reported_without_a_gpu():
    """Argument validation happens on the host before any launch."""
    from xequinet_amd import lib

    handle = lib.load()
    mul = lib.mul3((128, 64, 32))
    rc = handle.xeq_message_fwd(0, 10, 10, None, None, None, None, None, None, None, None, None, None, None, None,
                                0, 0, 64, 5.0, 128, mul, None, None, 0, None)
    assert rc == 1 and b"num_basis" in handle.xeq_last_error()
    rc = handle.xeq_message_fwd(0, 10, 10, None, None, None, None, None, None, None, None, None, None, None, None,
                                0, 0, 20, 5.0, 300, mul, None, None, 0, None)
    assert rc == 1 and b"256-channel" in handle.xeq_last_error()
    rc = handle.xeq_radial_fwd(0, None, 5, 7, 0, 20, 5.0, None, None, None, None, None)
    assert rc == 1 and b"not implemented" in handle.xeq_last_error()
    rc = handle.xeq_segment_sum(5, None, None, 3, 4, None, None)  # bad dtype code
    assert rc == 1
    # round-3 entries: training-pass kernels, the bounded CSR sort
    odd = lib.mul3((100, 64, 32))                                      # multiplicities outside the matrix-core forms
    assert handle.xeq_message_param_grad_mc_supported(lib.XEQ_F32, 0, 20, 128, mul) == 1
    assert handle.xeq_message_param_grad_mc_supported(lib.XEQ_F32, 0, 20, 128, odd) == 0
    assert handle.xeq_message_param_grad_mc_supported(lib.XEQ_F64, 0, 20, 128, mul) == 0
    assert handle.xeq_message_param_grad_mc_supported(lib.XEQ_F32, 1, 20, 128, mul) == 0       # gaussian, B = 20: 61 columns + harmonics > 64
    assert handle.xeq_param_basis_width(0, 20) == 64
    rc = handle.xeq_message_param_grad_mc(10, 10, None, None, None, None, None, None, None, 0, 20, 128, odd, 1, 1, None, 1, None, None)
    assert rc == 1 and b"multiples of 32" in handle.xeq_last_error()
    rc = handle.xeq_message_param_grad_mc(10, 10, None, None, None, None, None, None, None, 0, 20, 128, mul, 1, 1, None, 7, None, None)
    assert rc == 1 and b"xeq_message_param_grad_mc_parts" in handle.xeq_last_error()
    rc = handle.xeq_wgrad(None, 4, None, 4, 100, 8, 8, 0, 3, None, None)                       # rows strides below the widths
    assert rc == 1 and b"bad shape" in handle.xeq_last_error()
    rc = handle.xeq_wgrad(None, 8, None, 8, 100, 8, 8, 0, 3, None, None)                       # wrong chunk count
    assert rc == 1 and b"xeq_wgrad_chunks" in handle.xeq_last_error()
    assert handle.xeq_wgrad_chunks(18609, 576, 128) == 114 and handle.xeq_wgrad_chunks(5, 32, 32) == 1
    rc = handle.xeq_csr_by_key_bounded(None, 10, 5, None, None, 0, None, None, None)           # no device-side count
    assert rc == 1 and b"bad sizes" in handle.xeq_last_error()
    assert handle.xeq_message_wq_pcap(100, 1000) == 1400                                        # E + 4 N: a quad for every node without an edge
    # round-4 entries: the twice-differentiable training pass
    rc = handle.xeq_message_bwd_sbq(0, 10, 10, None, None, None, None, None, None, None, None, None, None, 40, 128, mul, None, None, None, None, 0, None)
    assert rc == 1 and b"num_basis" in handle.xeq_last_error()
    assert handle.xeq_message_q_wgrad_chunks(311994) == 610 and handle.xeq_message_q_wgrad_chunks(0) == 0
    rc = handle.xeq_message_q_wgrad(0, None, None, 1000, 20, 128, mul, 3, None, None)           # wrong chunk count (2)
    assert rc == 1 and b"n_chunks" in handle.xeq_last_error()
    rc = handle.xeq_message_q_wgrad(0, None, None, 1000, 20, 512, mul, 2, None, None)           # 960 filter rows
    assert rc == 1 and b"768" in handle.xeq_last_error()
    rc = handle.xeq_message_fwd_sb_pair(0, 10, 10, None, None, None, None, None, None, None, None, None, None, None, None, None, 20, 128, mul, None, None, 0, None)
    assert rc == 1 and b"cotangent operands" in handle.xeq_last_error()
    rc = handle.xeq_message_bwd_sbq_pair(0, 10, 10, None, None, None, None, None, None, None, None, None, None, None, None, None, 20, 300, mul, None, None, None, None, 0, None)
    assert rc == 1 and b"256-channel" in handle.xeq_last_error()
    rc = handle.xeq_train_norm(0, 0, 10, None, None, None, None, None, None, None, None, None, None, 128, mul, 1e-5, 1e-5, 2, None, None, None, None)
    assert rc == 1 and b"layout" in handle.xeq_last_error()
    rc = handle.xeq_train_norm(0, 1, 10, None, None, None, None, None, None, None, None, None, None, 128, mul, 1e-5, 1e-5, 0, None, None, None, None)
    assert rc == 1 and b"reverse form" in handle.xeq_last_error()
    rc = handle.xeq_train_uv(0, 1, 10, None, None, None, mul, 1e-5, None, None, None)
    assert rc == 1 and b"reverse form" in handle.xeq_last_error()
    rc = handle.xeq_train_out(7, 0, 10, None, None, None, None, None, None, None, None, 128, mul, None, None, None, None)   # bad dtype code
    assert rc == 1
    rc = handle.xeq_train_out(0, 0, 10, None, None, None, None, None, None, None, None, 128, lib.mul3((0, 0, 0)), None, None, None, None)
    assert rc == 1 and b"no channels" in handle.xeq_last_error()


def test_irreps_mirror():
    from xequinet_amd import o3

    ir = o3.Irreps("128x0e + 64x1o + 32x2e")
    assert ir.dim == 480 and ir.num_irreps == 224 and ir.mul3() == (128, 64, 32) and ir.lmax == 2
    assert str(ir) == "128x0e+64x1o+32x2e"
    assert o3.Irreps("16x1o").mul3() == (0, 16, 0)
    assert o3.Irreps("4x0e+4x0e+2x1o").simplify() == o3.Irreps("8x0e+2x1o")
    assert [(m, i.l, i.p) for m, i in o3.Irreps("1o+2x2e")] == [(1, 1, -1), (2, 2, 1)]
    with pytest.raises(NotImplementedError):
        o3.Irreps("8x3o").mul3()
    with pytest.raises(NotImplementedError):
        o3.Irreps("8x1o+8x0e").mul3()
    with pytest.raises(ValueError):
        o3.Irreps("8y0e")


def test_model_layout_matches_reference_state_dict():
    """parameter count and key layout of the default XPaiNN."""
    from xequinet_amd.nn import resolve_model

    model = resolve_model("xpainn")
    assert sum(p.numel() for p in model.parameters()) == 865141
    sd = model.state_dict()
    expect = {
        "mods.embedding.embedding.0.embed_ten": (87, 56),
        "mods.embedding.embedding.1.weight": (128, 56),
        "mods.embedding.rbf.freq": (1, 20),
        "mods.message_0.scalar_mlp.2.weight": (576, 128),
        "mods.message_2.rbf_lin.weight": (576, 20),
        "mods.message_1.o3norm.affine_weight": (224,),
        "mods.message_1.o3norm.affine_bias": (128,),
        "mods.message_1.o3norm.scalar_index": (128,),
        "mods.update_0.update_U.weight": (21504,),
        "mods.update_0.update_V.bias": (128,),
        "mods.update_2.dot_lin.weight": (128, 224),
        "mods.update_1.update_mlp.0.weight": (128, 352),
        "mods.update_1.update_mlp.2.weight": (480, 128),
        "mods.output_energy.out_mlp.0.weight": (64, 128),
        "mods.output_energy.out_mlp.2.weight": (1, 64),
    }
    for k, shape in expect.items():
        assert tuple(sd[k].shape) == shape, k
    assert list(model.mods.keys()) == ["embedding", "message_0", "update_0", "message_1", "update_1", "message_2",
                                       "update_2", "output_energy"]
    assert torch.all(sd["mods.embedding.embedding.0.embed_ten"][0] == 0)
    assert torch.all(sd["mods.embedding.embedding.1.bias"] == 0)  # nn/xpainn.py:48
    freq = sd["mods.embedding.rbf.freq"].double().numpy().ravel()
    np.testing.assert_allclose(freq, np.pi * np.arange(1, 21) / 5.0, rtol=1e-6)
    # a reference checkpoint carries e3nn bookkeeping entries: they are dropped, the rest is strict
    ref_sd = dict(sd)
    ref_sd["mods.message_0.rsh_conv.weight"] = torch.zeros(0)
    ref_sd["mods.message_0.rsh_conv.output_mask"] = torch.ones(480)
    ref_sd["mods.update_0.invariant.tp.weight"] = torch.zeros(0)
    model.load_reference_state_dict(ref_sd)
    ref_sd["mods.bogus.weight"] = torch.zeros(1)
    with pytest.raises(KeyError):
        model.load_reference_state_dict(ref_sd)


def test_factories_and_errors_mirror_reference():
    from xequinet_amd.nn import resolve_activation, resolve_cutoff, resolve_model, resolve_output, resolve_rbf

    with pytest.raises(NotImplementedError):
        resolve_model("so3krates")
    with pytest.raises(NotImplementedError):
        resolve_rbf("nope", 20, 5.0)
    with pytest.raises(NotImplementedError):
        resolve_cutoff("nope", 5.0)
    with pytest.raises(NotImplementedError):
        resolve_activation("gelu")
    with pytest.raises(NotImplementedError):
        resolve_output("dipole")
    assert isinstance(resolve_activation("silu", devide_x=True), torch.nn.Sigmoid)
    assert resolve_model("xpainn", action_blocks=1, node_dim=16, node_irreps="16x0e+8x1o").cutoff_radius == 5.0


def test_no_cpu_fallback():
    """Every op rejects CPU tensors loudly instead of computing on the host."""
    from xequinet_amd import o3, ops
    from xequinet_amd.nn import resolve_model

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o3.SphericalHarmonics("4x0e+2x1o", True, "component")(torch.randn(5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.EdgeGraph(torch.zeros((2, 4), dtype=torch.int64), 3)
    model = resolve_model("xpainn", action_blocks=1).eval()
    data = {"pos": torch.randn(4, 3), "atomic_numbers": torch.tensor([1, 6, 8, 1]),
            "edge_index": torch.tensor([[0, 1], [1, 0]])}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(data)


def test_batch_container():
    from xequinet_amd.data import XequiBatch

    b = XequiBatch(torch.randn(5, 3), torch.tensor([1, 1, 8, 6, 1]), torch.tensor([0, 3, 5]))
    assert b.num_graphs == 2 and b.batch.tolist() == [0, 0, 0, 1, 1]
    assert b.atomic_numbers.dtype == torch.int32
    assert set(b.to_dict()) == {"pos", "atomic_numbers", "ptr", "batch"}
    with pytest.raises(ValueError):
        XequiBatch(torch.randn(2, 3), torch.tensor([1, 1]), pbc=torch.tensor([True, True, True]))


# ------------------------------------------------------------------ units / MD front-end host logic
def test_unit_conversion_matches_reference_table():
    """utils/qc.py:13-114: every table entry and a set of compound conversions against factors produced by the
    reference's own functions (tests/golden/make_golden_units.py); malformed unit strings are refused."""
    import json

    from xequinet_amd.utils import check_unit, eval_unit, unit_conversion
    from xequinet_amd.utils.units import units

    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "units.json")))
    assert set(units) == set(g["table"])
    for k, v in g["table"].items():
        assert abs(units[k] / v - 1) < 1e-14, k
    for a, b, v in g["pairs"]:
        assert abs(unit_conversion(a, b) / v - 1) < 1e-14, (a, b)
    assert unit_conversion(None, "eV") == 1.0 and unit_conversion("eV", None) == 1.0 and unit_conversion("eV", "eV") == 1.0
    # published CODATA 2018 values, to the accuracy of the reference's constant set (mu0 = 4 pi 1e-7)
    assert abs(unit_conversion("Hartree", "eV") - 27.211386245988) < 1e-7
    assert abs(unit_conversion("Bohr", "Angstrom") - 0.529177210903) < 1e-9
    for bad in g["invalid"] + ["", "eV/", "(eV", "eV eV", "1/0"]:
        assert not check_unit(bad), bad
    with pytest.raises(ValueError):
        eval_unit("eV/parsec")
    assert eval_unit("2^3^2") == 512.0 and eval_unit("-2^2") == -4.0 and eval_unit("8/2/2") == 2.0   # Python's ** rules


def test_default_units_and_md_model_factors():
    from xequinet_amd import keys
    from xequinet_amd.utils import units as U

    saved = dict(U.DEFAULT_UNITS_MAP)
    try:
        with pytest.raises(ValueError):
            U.set_default_units({keys.FORCES: "eV/Angstrom"})
        with pytest.raises(ValueError):
            U.set_default_units({keys.TOTAL_ENERGY: "furlong"})
        U.set_default_units({keys.TOTAL_ENERGY: "kcal/mol"})
        d = U.get_default_units()
        assert d[keys.FORCES] == "kcal/mol/Angstrom" and d[keys.VIRIAL] == "kcal/mol/Angstrom^3"
        assert abs(U.unit_conversion(d[keys.FORCES], keys.LAMMPS_UNIT_STYLE["metal"][keys.FORCES]) - 0.0433641042) < 1e-9
    finally:
        U.DEFAULT_UNITS_MAP.clear()
        U.DEFAULT_UNITS_MAP.update(saved)
    assert set(keys.LAMMPS_UNIT_STYLE) == {"metal", "real", "electron"}


def test_ase_helpers_without_ase():
    from xequinet_amd.interface.ase_calculator import datapoint_from_ase, full_3x3_to_voigt_6_stress

    s = np.arange(9.0).reshape(3, 3)
    np.testing.assert_allclose(full_3x3_to_voigt_6_stress(s), [0, 4, 8, 6, 4, 2])

    class A:
        def get_pbc(self): return np.array([True, True, False])
        def get_cell(self): return np.diag([4.0, 5.0, 6.0])
        def get_atomic_numbers(self): return np.array([8, 1, 1])
        def get_positions(self, wrap=False): return np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 7.0], [3.9, 4.9, -1.0]])

    d = datapoint_from_ase(A(), torch.float64)
    assert d.pos.dtype == torch.float64 and d.atomic_numbers.dtype == torch.int32 and d.cell.shape == (1, 3, 3)
    assert d.pbc.tolist() == [[True, True, False]] and d.ptr.tolist() == [0, 3] and d.num_graphs == 1

    class M(A):
        def get_pbc(self): return np.array([False, False, False])

    d = datapoint_from_ase(M(), torch.float32)
    assert not hasattr(d, "cell") and not hasattr(d, "pbc") and d.pos.dtype == torch.float32


def test_torchscript_front_ends_script_save_and_reload_without_a_gpu(tmp_path):
    """compile_model (run/jit_script.py:28-86): the registered xeq:: operators give torch.jit.script something to see; the
    scripted LAMMPS / GROMACS front ends save with the reference's `_extra_files` and reload (no kernel runs here)."""
    import torch

    from xequinet_amd.interface.scripted import compile_model, load_torch_library
    from xequinet_amd.nn import resolve_model
    from xequinet_amd.utils import units as U

    load_torch_library()
    assert hasattr(torch.ops.xeq, "xpainn_eval") and hasattr(torch.ops.xeq, "radius_graph") and hasattr(torch.ops.xeq, "radius_graph_pbc")
    assert "Tensor pos, Tensor cell, Tensor pbc, float cutoff" in str(torch.ops.xeq.radius_graph_pbc.default._schema)
    schema = str(torch.ops.xeq.xpainn_eval.default._schema)
    assert "Tensor[] params" in schema and "-> Tensor[]" in schema
    saved = dict(U.DEFAULT_UNITS_MAP)
    U.set_default_units({"energy": "eV"})
    try:
        torch.manual_seed(0)
        model = resolve_model("xpainn", node_dim=32, node_irreps="32x0e+32x1o", num_basis=8, action_blocks=1, hidden_dim=16).eval()
        for mode in ("lmp", "gmx"):
            path = str(tmp_path / f"m-{mode}.jit")
            scripted = compile_model(model, mode=mode, unit_style="metal", output_file=path)
            assert "xpainn_eval" in scripted.core.code
            extra = {"cutoff_radius": "", "n_species": "", "periodic_table": "", "fusion_strategy": ""}
            again = torch.jit.load(path, _extra_files=extra)
            assert float(extra["cutoff_radius"]) == 5.0 and int(extra["n_species"]) == 87
            assert len(extra["periodic_table"].decode().split()) == 87
            assert again.core.flat.numel() == scripted.core.flat.numel()
        # the operator refuses host tensors: no CPU fallback behind the schema either
        import pytest
        with pytest.raises(RuntimeError, match="HIP"):
            scripted_l = compile_model(model, mode="lmp")
            scripted_l({"pos": torch.zeros(2, 3), "atomic_numbers": torch.ones(2, dtype=torch.int32),
                        "edge_index": torch.zeros(2, 0, dtype=torch.long)}, True, False)
    finally:
        U.DEFAULT_UNITS_MAP.clear()
        U.DEFAULT_UNITS_MAP.update(saved)


def test_models_and_irreps_survive_deepcopy_and_pickle():
    """copy.deepcopy(model) (EMA copies, the reference's checkpoint handling) must work: irreps are tuple subclasses."""
    import copy
    import pickle

    from xequinet_amd import o3, tp
    from xequinet_amd.nn import resolve_model

    for mod in (o3, tp):
        ir = mod.Irrep(1, -1)
        assert copy.deepcopy(ir) == ir and pickle.loads(pickle.dumps(ir)) == ir
        assert copy.deepcopy(mod.Irreps("128x0e + 64x1o + 32x2e")) == mod.Irreps("128x0e + 64x1o + 32x2e")
    model = resolve_model("xpainn")
    twin = copy.deepcopy(model)
    assert [k for k in twin.state_dict()] == [k for k in model.state_dict()]


def test_node_tile_split_covers_every_tile_once():
    """TileSplit (csrc/xeq_common.h): whole tiles one workgroup each in multiples of the CU count, a short remainder - or everything
    at MD sizes - shared by `split` workgroups; every (tile, part) pair appears exactly once in the grid."""
    import ctypes

    from xequinet_amd import lib

    L = lib.load()
    out = (ctypes.c_int64 * 3)()
    for tiles in (0, 1, 7, 100, 128, 129, 255, 256, 257, 320, 384, 385, 511, 576, 1000, 4608):
        for max_split in (1, 2, 5, 7):
            assert L.xeq_node_tile_split(tiles, max_split, out) == 0
            n_full, split, grid = out[0], out[1], out[2]
            assert 0 <= n_full <= tiles and 1 <= split <= max(1, max_split)
            assert grid == n_full + (tiles - n_full) * split
            seen = set()
            for b in range(grid):                       # the device-side decode, restated
                if b < n_full:
                    seen.add((b, 0))
                else:
                    r = b - n_full
                    seen.add((n_full + r // split, r % split))
            want = {(t, 0) for t in range(n_full)} | {(t, p) for t in range(n_full, tiles) for p in range(split)}
            assert seen == want
            if split > 1:                               # split tiles never outnumber the CUs they are spread over
                assert (tiles - n_full) * split <= 256
    assert L.xeq_node_tile_split(576, 5, out) == 0 and (out[0], out[1]) == (512, 4)     # QM9-1024: 64 tiles of the third round x 4
    assert L.xeq_node_tile_split(1, 5, out) == 0 and (out[0], out[1]) == (0, 5)         # aspirin: one tile, five workgroups


def test_host_cell_tables_match_the_device_operation_forms():
    """data/radius_graph._host_cell_tables (numpy, one round trip) against the tensor-operation forms it replaced in front of the
    periodic search (_image_counts, cartesian_prod + bmm, linalg.inv): image counts per axis, image table in cartesian_prod order,
    Cartesian image offsets, reciprocal rows, pruning thresholds, inverse cells -- random triclinic cells, mixed periodic flags."""
    import numpy as np
    import torch
    from xequinet_amd.data import radius_graph as rg

    g = torch.Generator().manual_seed(0)
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 2e-6)):
        for pbc in ([True, True, True], [True, False, True], [False, False, True]):
            cell = (torch.eye(3).unsqueeze(0) * torch.tensor([6.0, 9.0, 14.0]) + 1.5 * torch.randn(4, 3, 3, generator=g)).to(dtype)
            reps, n_cells, tab = rg._host_cell_tables(cell, pbc, 5.0, with_inverse=True)
            want_reps, (recip, thr, _) = rg._image_counts(cell, pbc, 5.0, with_prune=True)
            assert reps == want_reps
            axes = [torch.arange(-r, r + 1, dtype=dtype) for r in reps]
            grid = torch.cartesian_prod(*axes).reshape(-1, 3)
            assert n_cells == grid.shape[0] and torch.equal(tab["cell_offsets"], grid)
            offs = torch.bmm(grid.view(1, -1, 3).expand(4, -1, -1).contiguous(), cell)
            for name, got, want in (("pbc_offsets", tab["pbc_offsets"], offs), ("recip", tab["recip"], recip), ("thr", tab["thr"], thr),
                                    ("cell_inv", tab["cell_inv"], torch.linalg.inv(cell))):
                assert got.dtype == dtype and got.shape == want.shape, name
                scale = max(1.0, float(want.abs().max()))
                assert float((got - want).abs().max()) <= tol * scale, name
    _, _, tab = rg._host_cell_tables(cell, [True, True, True], 5.0, with_inverse=False)
    assert tab["cell_inv"] is None


def test_launch_policy_is_stated_once_in_the_c_abi():
    """xeq_message_auto_family / xeq_message_wq_edges_per_stream: host functions of the C ABI that the Python modules
    (ops.select_message_impl, ops._wq_edges_per_stream) and the registered operator both call -- no second copy of the rule."""
    import ctypes

    from xequinet_amd import lib

    L = lib.load()
    mul = (ctypes.c_int32 * 3)(128, 64, 32)
    fam = lambda dt, n, e, b=20: int(L.xeq_message_auto_family(dt, n, e, b, 128, mul))
    WQ, SB, GENERIC = 0, 1, 3
    assert fam(lib.XEQ_F32, 21, 360) == SB                    # one small molecule: launch-bound, no walk plan
    assert fam(lib.XEQ_F32, 18609, 311994) == WQ              # QM9-1024
    assert fam(lib.XEQ_F32, 1536, 82996) == WQ                # dense periodic box (round 3: wq wins there too)
    assert fam(lib.XEQ_F64, 18609, 311994) == SB              # f64
    assert fam(lib.XEQ_F32, 18609, 311994, 31) == WQ          # num_basis up to 31 (round 4: the wm family is gone)
    assert fam(lib.XEQ_F32, 18609, 311994, 32) == SB
    assert fam(lib.XEQ_F32, 3_000_000, 150_000_000) == GENERIC   # beyond every 32-bit offset
    assert fam(lib.XEQ_F32, 2_500_000, 40_000_000) in (SB, GENERIC)
    eps = lambda n, e: int(L.xeq_message_wq_edges_per_stream(n, e))
    assert eps(18609, 311994) == 80 and eps(5000, 119000) == 79 and eps(1000, 100000) == 80 and eps(192, 10390) == 54
    assert eps(21, 360) == 17 and eps(10, 20) == 16
    assert int(L.xeq_message_wq_win_ints(100)) >= 2 * (25 + 9)   # both stream classes' window tables
    # the few-row forms of the node-side products (bit-equal to the 32-row kernels): one limit, stated in the C ABI, overridable per call
    old = os.environ.pop("XEQ_SMALL_ROWS", None)
    try:
        assert int(L.xeq_small_rows_limit()) == 3584
        os.environ["XEQ_SMALL_ROWS"] = "0"
        assert int(L.xeq_small_rows_limit()) == 0
        os.environ["XEQ_SMALL_ROWS"] = "100000"
        assert int(L.xeq_small_rows_limit()) == 100000
    finally:
        os.environ.pop("XEQ_SMALL_ROWS", None)
        if old is not None:
            os.environ["XEQ_SMALL_ROWS"] = old
    import inspect

    from xequinet_amd import ops
    src = inspect.getsource(ops.select_message_impl) + inspect.getsource(ops._wq_edges_per_stream)
    assert "xeq_message_auto_family" in src and "xeq_message_wq_edges_per_stream" in src
    cpp = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xequinet_amd", "csrc", "xeq_torch.cpp")).read()
    assert "xeq_message_auto_family" in cpp and "xeq_message_wq_edges_per_stream" in cpp and "E < 4096" not in cpp


def test_linear_operator_is_differentiable_to_second_order_on_the_host():
    """``xeq::linear`` (csrc/xeq_torch.cpp): the node pair y = x W^T + b / a^T b is closed under differentiation; on host tensors the
    row reduction falls to the library product, the graph structure is the one the GPU pass runs."""
    import torch
    from torch.autograd import gradcheck, gradgradcheck

    from xequinet_amd.interface import scripted

    scripted.load_torch_library()
    g = torch.Generator().manual_seed(0)
    x, W, b = (torch.randn(*shape, generator=g, dtype=torch.float64).requires_grad_() for shape in ((7, 5), (3, 5), (3,)))
    assert gradcheck(torch.ops.xeq.linear, (x, W, b)) and gradgradcheck(torch.ops.xeq.linear, (x, W, b))
    assert gradcheck(lambda a, c: torch.ops.xeq.linear(a, c, None), (x, W)) and gradgradcheck(lambda a, c: torch.ops.xeq.linear(a, c, None), (x, W))
    assert torch.allclose(torch.ops.xeq.linear(x, W, b), torch.nn.functional.linear(x, W, b), rtol=0, atol=1e-14)


def test_matrix_core_objects_hold_no_packed_fp32_instructions():
    """Every object with v_mfma in it is built with -packed-fp32-ops off (csrc/build.py: MFMA_SOURCES; the sporadic wrong rows of
    round 4, profiles/r04_nodeblock.txt item 9c): the disassembly of the built objects holds no v_pk_{fma,add,mul}_f32 there, and
    no object outside that list holds a matrix-core instruction."""
    from xequinet_amd.csrc import build

    build.build(verbose=False)
    build.check_no_packed()
    for src in build.MFMA_SOURCES:
        pk, mfma = build.packed_fp32_counts(src)
        assert pk == 0 and mfma > 0, (src, pk, mfma)


def test_launch_counter_is_exported_and_starts_without_a_gpu():
    from xequinet_amd import lib

    assert lib.launch_count() >= 0


def test_graphed_train_step_checks_the_edge_capacity_on_the_host():
    """``GraphedTrainStep.__call__(ptr_host=...)`` refuses a batch that may overflow the captured edge capacity BEFORE anything is
    loaded (round-5 advisor, medium: the check raised NameError because ``runtime`` was imported in ``__init__`` only)."""
    import types

    from xequinet_amd import runtime, train

    step = object.__new__(train.GraphedTrainStep)
    step._gs = types.SimpleNamespace(n_edges=100)
    ptr_host = np.array([0, 12, 24])                          # 2 x 12 x 11 = 264 ordered pairs > 100
    assert runtime.pair_capacity(ptr_host) == 264
    with pytest.raises(ValueError, match="capacity is 100"):
        step(None, None, torch.tensor(ptr_host), None, ptr_host=ptr_host)


def test_pack_cache_helper_rebuilds_exactly_when_its_key_moves():
    """lib.cached, the one packed-weight cache of the Python front: a rebuild when a tensor is modified in place, when its storage is
    replaced, when the pack epoch is bumped, when the flags change and when a tensor is absent instead of present -- and only then."""
    from xequinet_amd import lib

    class Owner:
        pass

    owner, builds = Owner(), []
    w, b = torch.randn(4, 3), torch.randn(4)

    def get(tensors, extra=(), slot="_pack"):
        def build():
            assert not torch.is_grad_enabled()
            builds.append(slot)
            return len(builds)

        return lib.cached(owner, slot, tensors, build, extra)

    assert get((w, b)) == 1 and get((w, b)) == 1 and len(builds) == 1        # nothing changed: no rebuild
    with torch.no_grad():
        b.add_(1.0)                                                          # (a) in place: the version counter moves
    assert get((w, b)) == 2 and get((w, b)) == 2
    version, address = w._version, w.data_ptr()
    w.data = w.data.clone()                                                  # (b) a new storage under the same tensor and version
    assert w._version == version and w.data_ptr() != address
    assert get((w, b)) == 3 and get((w, b)) == 3
    lib.bump_pack_epoch()                                                    # (c) parameters changed behind autograd's back
    assert get((w, b)) == 4 and get((w, b)) == 4
    assert get((w, b), (True,)) == 5 and get((w, b), (True,)) == 5           # (d) another form of the pack
    assert get((w, b), (False,)) == 6
    assert get((w, None)) == 7 and get((w, None)) == 7 and get((w, b)) == 8  # an absent tensor is not a present one
    assert get((w, b), slot="_other") == 9 and get((w, b)) == 8              # slots do not share entries
    assert owner._pack[1] == 8 and owner._pack[0] == lib.pack_key((w, b))
