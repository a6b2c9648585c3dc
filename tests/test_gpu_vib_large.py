"""The eigensolver above the LDS cap on the GPU (xeq_vib_eigh_large, ``harmonic_analysis(..., large="kernel")``) against numpy and
the oracle of tests/vib_oracle.py.

Bounds: those of tests/test_gpu_vib.py, unchanged.  The eigensolver alone: 4 m 2^-52 max|lambda| for eigenvalues and residuals and
4 m 2^-52 for V^T V - I (the numpy restatement of the kernel, tests/vib_large_oracle.py, needs 0.02-0.15 of the unit); two kernels on
one matrix: 8 m 2^-52 max|lambda|, both sides carry 4.  The pipeline: the four bounds of test_pipeline_against_the_oracle -- eigenvalues
and modes against Q in the same unit, derived quantities at 1e-10 relative (the synthetic spectra keep every eigenvalue above 5 % of the
largest), vectors at 8 m 2^-52 max(1, sigma / smallest gap).  The graph above the larger cap takes ``torch.linalg.eigh``, whose backward
error is relative to the matrix it is handed, |M| = sigma: its eigenvalues are held to 4 m 2^-52 sigma and its wavenumbers to 1e-10 plus
that bound carried through the square root (dl / 2 l <= bound / l), as test_vibrations_on_a_small_model does.  Every ratio is printed
before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

from tests import vib_oracle as vo
from tests.test_vib_large_host import matrices, ratios
from xequinet_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
U52 = 2.0 ** -52
UNITS = dict(energy_unit="eV", length_unit="Angstrom")


def _vib():
    from xequinet_amd import vibrations

    return vibrations


def _run(entry, mats, max_dim=None):
    """``entry`` (xeq_vib_eigh or xeq_vib_eigh_large) on a list of symmetric numpy matrices -> rc, (eigenvalues, vectors [m, m] rows) per
    matrix, sweeps, status, and the input as the device holds it after the launch."""
    dims = [a.shape[0] for a in mats]
    mat_off = np.concatenate([[0], np.cumsum([d * d for d in dims])])
    val_off = np.concatenate([[0], np.cumsum(dims)])
    flat = torch.tensor(np.concatenate([a.ravel() for a in mats]), dtype=torch.float64, device=DEV)
    d_mat, d_val = torch.tensor(mat_off[:-1], device=DEV), torch.tensor(val_off[:-1], device=DEV)
    d_dim = torch.tensor(dims, dtype=torch.int32, device=DEV)
    w = torch.full((int(val_off[-1]),), float("nan"), dtype=torch.float64, device=DEV)
    v = torch.full((int(mat_off[-1]),), float("nan"), dtype=torch.float64, device=DEV)
    sweeps = torch.full((len(mats),), -1, dtype=torch.int32, device=DEV)
    status = torch.full((len(mats),), -1, dtype=torch.int32, device=DEV)
    rc = getattr(lib.load(), entry)(lib.ptr(flat), lib.ptr(d_mat), lib.ptr(d_val), lib.ptr(d_dim), len(mats), max(dims) if max_dim is None else max_dim,
                                    lib.ptr(w), lib.ptr(v), lib.ptr(sweeps), lib.ptr(status), lib.stream())
    torch.cuda.synchronize()
    w, v = w.cpu().numpy(), v.cpu().numpy()
    pairs = [(w[val_off[g] : val_off[g + 1]], v[mat_off[g] : mat_off[g + 1]].reshape(dims[g], dims[g])) for g in range(len(mats))]
    return rc, pairs, sweeps.cpu().tolist(), status.cpu().tolist(), flat.cpu().numpy()


def _check_contract(tag, A, w, Vt, sw, st, min_sweeps=0):
    m = A.shape[0]
    e_val, e_res, e_orth = ratios(A, w, Vt)
    print(f"vib_eigh_large {tag}: iterations {sw:2d}, |dlambda| {e_val:.3f}, residual {e_res:.3f}, orthogonality {e_orth:.3f}  (units of m 2^-52 [max|lambda|])")
    assert st == 0 and min_sweeps <= sw <= 30
    assert (np.diff(w) >= 0).all()
    assert e_val <= 4 and e_res <= 4 and e_orth <= 4
    lead = np.abs(Vt).argmax(axis=1)
    assert (Vt[np.arange(m), lead] > 0).all()              # the largest-magnitude component of every vector is positive


# ------------------------------------------------------------------------------------------------------------ the eigensolver alone
@pytest.mark.parametrize("m", [97, 98, 99, 255, 256, 257, 513, 768])
def test_eigh_large_against_numpy(m):
    named = matrices(m)
    mats = [A for _, A in named]
    first = lib.launch_count()
    rc, got, sweeps, status, after = _run("xeq_vib_eigh_large", mats)
    assert rc == 0 and lib.launch_names(first) == ["xeq_vib_eigh_large"]
    assert np.array_equal(after, np.concatenate([A.ravel() for A in mats]))          # the input is only read
    for (name, A), (w, Vt), sw, st in zip(named, got, sweeps, status):
        _check_contract(f"m={m:3d} {name:11s}", A, w, Vt, sw, st, min_sweeps=1)


def test_eigh_large_refuses_a_dimension_beyond_its_cap_without_a_launch():
    first = lib.launch_count()
    rc, _, sweeps, status, _ = _run("xeq_vib_eigh_large", [np.eye(lib.VIB_LARGE_MAX_DIM + 1)])
    assert rc == 1 and b"XEQ_VIB_LARGE_MAX_DIM" in lib.load().xeq_last_error()
    assert lib.launch_count() == first and sweeps == [-1] and status == [-1]


def test_eigh_large_on_structured_matrices():
    m = 129
    rng = np.random.default_rng(129)
    diag = np.diag(rng.permutation(np.arange(1.0, m + 1)) - 40.0)
    tri = np.diag(rng.standard_normal(m)) + np.diag(rng.standard_normal(m - 1), 1)
    tri = np.triu(tri) + np.triu(tri, 1).T
    block = np.zeros((m, m))
    for a, b in ((0, 64), (64, m)):
        B = rng.standard_normal((b - a, b - a))
        block[a:b, a:b] = 0.5 * (B + B.T)
    named = [("diagonal", diag), ("tridiagonal", tri), ("two blocks", block), ("identity", np.eye(m))]
    rc, got, sweeps, status, _ = _run("xeq_vib_eigh_large", [A for _, A in named])
    assert rc == 0
    for (name, A), (w, Vt), sw, st in zip(named, got, sweeps, status):
        _check_contract(f"m={m} {name:11s}", A, w, Vt, sw, st)
    assert sweeps[0] == 0 and sweeps[3] == 0                                           # nothing to iterate on
    assert np.array_equal(got[0][0], np.sort(np.diag(diag))) and np.array_equal(got[3][1], np.eye(m))
    assert np.array_equal(np.abs(got[0][1]).argmax(axis=1), np.argsort(np.diag(diag))) and set(np.unique(got[0][1])) == {0.0, 1.0}


@pytest.mark.parametrize("m", [1, 2, 63, 96])
def test_both_kernels_on_one_matrix(m):
    rng = np.random.default_rng(300 + m)
    A = rng.standard_normal((m, m))
    A = 0.5 * (A + A.T)
    _, ((w_small, _),), _, st_small, _ = _run("xeq_vib_eigh", [A])
    _, ((w, Vt),), (sw,), (st,), _ = _run("xeq_vib_eigh_large", [A])
    _check_contract(f"m={m:3d} below the cap", A, w, Vt, sw, st)
    top = np.abs(np.linalg.eigvalsh(A)).max()
    diff = np.abs(w - w_small).max() / (m * U52 * top)
    print(f"vib_eigh_large m={m:3d}: against xeq_vib_eigh {diff:.3f} of m 2^-52 max|lambda|")
    assert st_small == [0] and diff <= 8


def test_eigh_large_ragged_batch_is_independent_of_its_composition():
    rng = np.random.default_rng(11)
    mats = []
    for m in (257, 97, 768, 130, 99):
        A = rng.standard_normal((m, m))
        mats.append(0.5 * (A + A.T))
    _, batch, sw_b, st_b, _ = _run("xeq_vib_eigh_large", mats)
    _, rev, sw_r, _, _ = _run("xeq_vib_eigh_large", mats[::-1])
    assert st_b == [0] * len(mats)
    for g, A in enumerate(mats):
        _, (alone,), sw_a, _, _ = _run("xeq_vib_eigh_large", [A])
        for other, sw in ((batch[g], sw_b[g]), (rev[len(mats) - 1 - g], sw_r[len(mats) - 1 - g])):
            assert np.array_equal(alone[0], other[0]) and np.array_equal(alone[1], other[1]) and sw_a[0] == sw


# ------------------------------------------------------------------------------------------------------------ the pipeline
SIZES = [5, 33, 21, 40, 64, 86]
SOLVERS = ["kernel", "large", "kernel", "large", "large", "large"]


def _graph(n, seed, scale):
    pos, mass = vo.molecule(n, seed)
    H = vo.synthetic_hessian(pos, mass, 40 + seed, scale=scale)
    return pos, mass, H, vo.harmonic(H, pos, mass)


@functools.lru_cache(maxsize=None)
def _batch():
    """The ragged batch (host numpy) and its oracle results, computed once and shared: do not change them."""
    return tuple(_graph(n, 110 + g, [1.0, 30.0, 0.2][g % 3]) for g, n in enumerate(SIZES))


def _device_inputs(graphs, dtype=torch.float64):
    H = [torch.tensor(g[2], dtype=dtype, device=DEV) for g in graphs]
    pos = torch.tensor(np.concatenate([g[0] for g in graphs]), dtype=torch.float64, device=DEV)
    mass = torch.tensor(np.concatenate([g[1] for g in graphs]), dtype=torch.float64, device=DEV)
    return H, pos, mass


def _analyse(graphs, dtype=torch.float64, **kw):
    H, pos, mass = _device_inputs(graphs, dtype)
    return _vib().harmonic_analysis(H, pos, mass, **dict(UNITS, **kw))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.abs(want)).max())


def _against_the_oracle(res, graphs, tensor_graphs=()):
    """The bounds of tests/test_gpu_vib.py::test_pipeline_against_the_oracle on every graph; a graph of ``tensor_graphs`` has its
    eigenvalues and wavenumbers held to the tensor solver's bound (the module's docstring)."""
    G = len(graphs)
    assert res.status.tolist() == [0] * G and res.n_imaginary.tolist() == [0] * G and res.n_tr.tolist() == [g[3]["n_tr"] for g in graphs]
    sums = torch.zeros((G, 4), dtype=torch.float64, device=DEV)
    lib.call("xeq_vib_thermo_sums", lib.ptr(res.vib_temperature), lib.ptr(res.eigenvalue), lib.ptr(res.mode_ptr), G, 298.15, lib.ptr(sums), lib.stream())
    sums = sums.cpu().numpy()
    sigma = res.sigma.tolist()
    for g, (pos, mass, H, ref) in enumerate(graphs):
        n, m = len(mass), 3 * len(mass)
        lam = res.eigenvalues(g).cpu().numpy()
        k = len(ref["eigenvalue"])
        assert lam.shape == (k,) and tuple(res.modes(g).shape) == (k, n, 3)
        top = np.abs(ref["eigenvalue"]).max()
        e_val = np.abs(lam - ref["eigenvalue"]).max() / (m * U52 * top)
        nm = res.modes(g).cpu().numpy()
        mw = (nm * np.sqrt(mass)[None, :, None]).reshape(k, m)                         # the unit mass-weighted vectors
        Q = res.rigid_basis(g).cpu().numpy()
        e_q = np.abs(mw @ Q.T).max() / (m * U52)
        e_qq = np.abs(Q @ Q.T - np.eye(len(Q))).max() / (m * U52)
        mine = vo.from_modes(lam, mw.T, mass)
        gap = np.diff(ref["eigenvalue"]).min()
        want = ref["modes"].T
        sign = np.sign(np.einsum("ki,ki->k", mw, want))
        e_vec = np.abs(mw - sign[:, None] * want).max()
        tol_vec = 8 * m * U52 * max(1.0, sigma[g] / gap)
        print(f"vib large pipeline graph {g} n={n:3d} ({res.solver[g]}, sweeps {res.sweeps[g].item()}): |dlambda| {e_val:.3f}, modes.Q {e_q:.3f}, Q Q^T - I {e_qq:.3f} "
              f"(units of m 2^-52), modes vs oracle {e_vec:.2e} (bound {tol_vec:.2e}), sigma / top {sigma[g] / top:.2f}")
        f_got, f_ref = res.frequencies(g).cpu().numpy(), ref["freq_wavenumber"]
        if g in tensor_graphs:
            bound = 4 * m * U52 * sigma[g]
            assert np.abs(lam - ref["eigenvalue"]).max() <= bound
            assert (np.abs(f_got - f_ref) <= (1e-10 + bound / np.abs(ref["eigenvalue"])) * np.abs(f_ref)).all()
        else:
            assert e_val <= 4
            assert _rel(f_got, f_ref) <= 1e-10
            assert _rel(res.vib_temperature[res._rows(g)].cpu().numpy(), ref["vib_temperature"]) <= 1e-10
            assert _rel(sums[g], vo.thermo_sums(ref["vib_temperature"], ref["eigenvalue"], 298.15)) <= 1e-10
        assert e_q <= 4 and e_qq <= 4
        assert _rel(res.reduced_mass[res._rows(g)].cpu().numpy(), mine["reduced_mass"]) <= 4 * m * U52
        assert _rel(res.force_const[res._rows(g)].cpu().numpy(), mine["force_const"]) <= 4 * m * U52
        assert e_vec <= tol_vec


def test_pipeline_with_the_large_kernel_against_the_oracle():
    graphs = _batch()
    first = lib.launch_count()
    res = _analyse(graphs, large="kernel")
    assert lib.launch_names(first) == ["xeq_vib_project", "xeq_vib_eigh", "xeq_vib_eigh_large", "xeq_vib_finish"]
    assert res.solver == SOLVERS and max(res.sweeps.tolist()) <= 30 and min(res.sweeps.tolist()) >= 1
    _against_the_oracle(res, graphs)
    default = _analyse(graphs)
    assert default.solver == [s if s == "kernel" else "tensor" for s in SOLVERS]
    for g in (0, 2):                                                                  # the small graphs: bit for bit what a default call gives
        assert torch.equal(res.eigenvalues(g), default.eigenvalues(g)) and torch.equal(res.modes(g), default.modes(g))
        assert torch.equal(res.frequencies(g), default.frequencies(g)) and res.sweeps[g].item() == default.sweeps[g].item()
    big = tuple(g for g, s in zip(graphs, SOLVERS) if s == "large")
    first = lib.launch_count()
    only = _analyse(big, large="kernel")
    assert lib.launch_names(first) == ["xeq_vib_project", "xeq_vib_eigh_large", "xeq_vib_finish"] and only.solver == ["large"] * len(big)
    at = [g for g, s in enumerate(SOLVERS) if s == "large"]
    for h, g in enumerate(at):                                                        # and a graph does not depend on its batch
        assert torch.equal(only.eigenvalues(h), res.eigenvalues(g)) and torch.equal(only.modes(h), res.modes(g))
        assert only.sweeps[h].item() == res.sweeps[g].item()


def test_the_two_large_solvers_agree():
    graphs = _batch()
    a, b = _analyse(graphs, large="kernel"), _analyse(graphs, large="tensor")
    assert b.solver == [s if s == "kernel" else "tensor" for s in SOLVERS]
    for g in range(len(graphs)):
        diff = _rel(a.frequencies(g).cpu().numpy(), b.frequencies(g).cpu().numpy())
        print(f"vib large graph {g} ({a.solver[g]} / {b.solver[g]}): wavenumbers differ by {diff:.2e} relative")
        assert diff <= 1e-10


def test_a_graph_above_the_large_cap_keeps_the_tensor_solver():
    graphs = (_batch()[3], _graph(257, 131, 1.0))
    first = lib.launch_count()
    res = _analyse(graphs, large="kernel")
    assert lib.launch_names(first) == ["xeq_vib_project", "xeq_vib_eigh_large", "xeq_vib_finish"]
    assert res.solver == ["large", "tensor"] and res.sweeps[1].item() == 0
    _against_the_oracle(res, graphs, tensor_graphs=(1,))


def test_f32_hessians_match_their_widened_copy_bit_for_bit_with_the_large_kernel():
    graphs = _batch()
    a = _analyse(graphs, torch.float32, large="kernel")
    H, pos, mass = _device_inputs(graphs, torch.float32)
    b = _vib().harmonic_analysis([h.double() for h in H], pos, mass, large="kernel", **UNITS)
    assert a.solver == SOLVERS
    for name in ("eigenvalue", "freq_wavenumber", "vib_temperature", "reduced_mass", "force_const", "norm_mode", "sigma", "moments", "sweeps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ------------------------------------------------------------------------------------------------------------ a non-finite Hessian (last)
def test_a_nan_ends_as_a_status_and_leaves_the_other_graphs_alone():
    graphs = _batch()
    H, pos, mass = _device_inputs(graphs)
    H[3][7, 11, 1, 2] = float("nan")
    with pytest.raises(FloatingPointError, match=r"graphs \[3\]"):                      # that graph and no other
        _vib().harmonic_analysis(H, pos, mass, large="kernel", **UNITS)
    # the entry itself: the matrices either side of a non-finite one come out as they do alone
    rng = np.random.default_rng(12)
    mats = []
    for m in (120, 120, 99):
        A = rng.standard_normal((m, m))
        mats.append(0.5 * (A + A.T))
    mats[1][5, 60] = mats[1][60, 5] = float("nan")
    rc, got, sweeps, status, _ = _run("xeq_vib_eigh_large", mats)
    assert rc == 0 and status == [0, 1, 0] and 0 <= sweeps[1] <= 30
    for g in (0, 2):
        _, (alone,), sw, _, _ = _run("xeq_vib_eigh_large", [mats[g]])
        assert np.array_equal(alone[0], got[g][0]) and np.array_equal(alone[1], got[g][1]) and sw[0] == sweeps[g]
        _check_contract(f"m={mats[g].shape[0]} beside a NaN", mats[g], got[g][0], got[g][1], sweeps[g], status[g], min_sweeps=1)
