"""Harmonic analysis on the GPU (xequinet_amd/vibrations.py, csrc/xeq_vib.hip) against the numpy oracle of tests/vib_oracle.py.

Bounds.  Eigenvalues, residuals and orthogonality of the eigensolver: 4 m 2^-52 max |lambda| (4 m 2^-52 for V^T V - I), the standard
backward-error form m u |M| with a factor 4; a round-robin Jacobi restated in numpy needed 0.05-0.5, 0.03-0.4 and 0.2-1.7 of the unit
m 2^-52 (max |lambda|) on the same classes of spectra.  Every test prints the ratios it measured before it asserts (profiles/vib_parity.txt
keeps a run's figures).  Derived quantities: 1e-10 relative -- the synthetic spectra keep every eigenvalue above 5 % of the largest, so
sqrt and the thermochemistry sums are well conditioned, and 4 m 2^-52 <= 1e-13 leaves three decades.  Eigenvectors against the oracle:
a backward error E moves an eigenvector by |E| / gap, both sides carry one, and |E| <= 4 m 2^-52 sigma for M (largest eigenvalue:
the shift sigma): 8 m 2^-52 max(1, sigma / smallest gap), on the unit mass-weighted vectors.
"""
import functools

import numpy as np
import pytest
import torch

from tests import vib_oracle as vo
from xequinet_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
U52 = 2.0 ** -52
UNITS = dict(energy_unit="eV", length_unit="Angstrom")


def _vib():
    from xequinet_amd import vibrations

    return vibrations


# ------------------------------------------------------------------------------------------------------------ the eigensolver alone
def _run_eigh(mats, max_dim=None):
    """xeq_vib_eigh on a list of symmetric numpy matrices -> (eigenvalues, vectors [m, m] rows) per matrix, sweeps, status."""
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
    rc = lib.load().xeq_vib_eigh(lib.ptr(flat), lib.ptr(d_mat), lib.ptr(d_val), lib.ptr(d_dim), len(mats), max(dims) if max_dim is None else max_dim,
                                 lib.ptr(w), lib.ptr(v), lib.ptr(sweeps), lib.ptr(status), lib.stream())
    torch.cuda.synchronize()
    w, v = w.cpu().numpy(), v.cpu().numpy()
    return rc, [(w[val_off[g] : val_off[g + 1]], v[mat_off[g] : mat_off[g + 1]].reshape(dims[g], dims[g])) for g in range(len(mats))], \
        sweeps.cpu().tolist(), status.cpu().tolist()


def _spectra(m, rng):
    return {"separated": np.arange(1, m + 1) - m / 3.0, "six decades": 10.0 ** rng.uniform(-6.0, 0.0, m),
            "repeated": np.repeat(np.arange(1, m // 3 + 2), 3)[:m].astype(float)}


@pytest.mark.parametrize("m", [1, 2, 3, 9, 12, 15, 63, 87, 96])
def test_eigh_against_numpy(m):
    rng = np.random.default_rng(100 + m)
    names, mats = [], []
    for name, lam in _spectra(m, rng).items():
        U = np.linalg.qr(rng.standard_normal((m, m)))[0]
        A = (U * lam) @ U.T
        names.append(name)
        mats.append(0.5 * (A + A.T))
    first = lib.launch_count()
    rc, got, sweeps, status = _run_eigh(mats)
    assert rc == 0 and lib.launch_names(first) == ["xeq_vib_eigh"]
    for name, A, (w, Vt), sw, st in zip(names, mats, got, sweeps, status):
        ref = np.linalg.eigvalsh(A)
        top = np.abs(ref).max()
        e_val = np.abs(w - ref).max() / (m * U52 * top)
        e_res = np.abs(A @ Vt.T - Vt.T * w).max() / (m * U52 * top)
        e_orth = np.abs(Vt @ Vt.T - np.eye(m)).max() / (m * U52)
        print(f"vib_eigh m={m:2d} {name:11s}: sweeps {sw:2d}, |dlambda| {e_val:.3f}, residual {e_res:.3f}, orthogonality {e_orth:.3f}  (units of m 2^-52 [max|lambda|])")
        assert st == 0 and 0 <= sw <= 30
        assert (np.diff(w) >= 0).all()
        assert e_val <= 4 and e_res <= 4 and e_orth <= 4
        lead = np.abs(Vt).argmax(axis=1)
        assert (Vt[np.arange(m), lead] > 0).all()              # the largest-magnitude component of every vector is positive


def test_eigh_refuses_a_dimension_beyond_the_cap_without_a_launch():
    A = np.eye(97)
    first = lib.launch_count()
    rc, _, sweeps, status = _run_eigh([A])
    assert rc == 1 and b"XEQ_VIB_MAX_DIM" in lib.load().xeq_last_error()
    assert lib.launch_count() == first and sweeps == [-1] and status == [-1]


def test_eigh_ragged_batch_is_independent_of_its_composition():
    rng = np.random.default_rng(7)
    mats = []
    for m in (96, 1, 15, 2, 63, 9):
        A = rng.standard_normal((m, m))
        mats.append(0.5 * (A + A.T))
    _, batch, sw_b, _ = _run_eigh(mats)
    _, rev, sw_r, _ = _run_eigh(mats[::-1])
    for g, A in enumerate(mats):
        _, (alone,), sw_a, _ = _run_eigh([A])
        for other, sw in ((batch[g], sw_b[g]), (rev[len(mats) - 1 - g], sw_r[len(mats) - 1 - g])):
            assert np.array_equal(alone[0], other[0]) and np.array_equal(alone[1], other[1]) and sw_a[0] == sw


# ------------------------------------------------------------------------------------------------------------ the pipeline
SIZES = [1, 2, 3, 3, 5, 21, 29, 32, 33]
LINEAR = [False, True, True, False, False, False, False, False, False]


@functools.lru_cache(maxsize=None)
def _batch():
    """The ragged batch (host numpy) and its oracle results, computed once and shared: do not change them."""
    graphs = []
    for g, (n, lin) in enumerate(zip(SIZES, LINEAR)):
        pos, mass = vo.molecule(n, 10 + g, linear=lin)
        H = vo.synthetic_hessian(pos, mass, 50 + g, scale=[1.0, 30.0, 0.2][g % 3])
        graphs.append((pos, mass, H, vo.harmonic(H, pos, mass)))
    return tuple(graphs)


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
    if want.size == 0:
        assert got.size == 0
        return 0.0
    return float((np.abs(got - want) / np.abs(want)).max())


def test_pipeline_against_the_oracle():
    graphs = _batch()
    res = _analyse(graphs)
    G = len(graphs)
    assert res.n_tr.tolist() == [g[3]["n_tr"] for g in graphs] == [3, 5, 5, 6, 6, 6, 6, 6, 6]
    assert res.rotor.tolist() == [g[3]["rotor"] for g in graphs] == [0, 1, 1, 2, 2, 2, 2, 2, 2]
    assert res.mode_ptr.tolist() == np.concatenate([[0], np.cumsum([3 * n - t for n, t in zip(SIZES, [3, 5, 5, 6, 6, 6, 6, 6, 6])])]).tolist()
    assert res.solver == ["kernel"] * 8 + ["tensor"] and res.status.tolist() == [0] * G and max(res.sweeps.tolist()) <= 30
    assert res.n_imaginary.tolist() == [0] * G
    sums = torch.zeros((G, 4), dtype=torch.float64, device=DEV)
    lib.call("xeq_vib_thermo_sums", lib.ptr(res.vib_temperature), lib.ptr(res.eigenvalue), lib.ptr(res.mode_ptr), G, 298.15, lib.ptr(sums), lib.stream())
    sums = sums.cpu().numpy()
    sigma = res.sigma.tolist()
    for g, (pos, mass, H, ref) in enumerate(graphs):
        n, m = len(mass), 3 * len(mass)
        lam = res.eigenvalues(g).cpu().numpy()
        k = len(ref["eigenvalue"])
        assert lam.shape == (k,) and tuple(res.modes(g).shape) == (k, n, 3)
        assert _rel(res.moments[g].cpu().numpy()[ref["moments"] > 1e-6 * max(ref["moments"].max(), 1e-300)],
                    ref["moments"][ref["moments"] > 1e-6 * max(ref["moments"].max(), 1e-300)]) <= 1e-10
        assert abs(res.mass_tot[g].item() / mass.sum() - 1) <= 1e-14
        if k == 0:
            assert (sums[g] == 0).all()
            continue
        top = np.abs(ref["eigenvalue"]).max()
        e_val = np.abs(lam - ref["eigenvalue"]).max() / (m * U52 * top)
        nm = res.modes(g).cpu().numpy()
        mw = (nm * np.sqrt(mass)[None, :, None]).reshape(k, m)                         # the unit mass-weighted vectors
        Q = res.rigid_basis(g).cpu().numpy()
        e_q = np.abs(mw @ Q.T).max() / (m * U52)
        e_qq = np.abs(Q @ Q.T - np.eye(len(Q))).max() / (m * U52)
        mine = vo.from_modes(lam, mw.T, mass)
        gap = np.diff(ref["eigenvalue"]).min() if k > 1 else np.inf
        width = ref["eigenvalue"].max() - ref["eigenvalue"].min()
        want = ref["modes"].T
        sign = np.sign(np.einsum("ki,ki->k", mw, want))
        e_vec = np.abs(mw - sign[:, None] * want).max()
        tol_vec = 8 * m * U52 * max(1.0, sigma[g] / gap)
        print(f"vib pipeline graph {g} n={n:2d} ({res.solver[g]}, sweeps {res.sweeps[g].item()}): |dlambda| {e_val:.3f}, modes.Q {e_q:.3f}, Q Q^T - I {e_qq:.3f} "
              f"(units of m 2^-52), modes vs oracle {e_vec:.2e} (bound {tol_vec:.2e}), sigma / top {sigma[g] / top:.2f}")
        assert e_val <= 4 and e_q <= 4 and e_qq <= 4
        assert _rel(res.frequencies(g).cpu().numpy(), ref["freq_wavenumber"]) <= 1e-10
        assert _rel(res.vib_temperature[res._rows(g)].cpu().numpy(), ref["vib_temperature"]) <= 1e-10
        assert _rel(sums[g], vo.thermo_sums(ref["vib_temperature"], ref["eigenvalue"], 298.15)) <= 1e-10
        assert _rel(res.reduced_mass[res._rows(g)].cpu().numpy(), mine["reduced_mass"]) <= 4 * m * U52
        assert _rel(res.force_const[res._rows(g)].cpu().numpy(), mine["force_const"]) <= 4 * m * U52
        assert gap > 1e-6 * width or k == 1
        assert e_vec <= tol_vec


def test_one_negative_eigenvalue_is_one_imaginary_mode():
    pos, mass = vo.molecule(5, 14)
    H = vo.synthetic_hessian(pos, mass, 77, negative=True)
    ref = vo.harmonic(H, pos, mass)
    assert ref["n_imaginary"] == 1 and ref["freq_wavenumber"][0] < 0
    res = _analyse(((pos, mass, H, ref),))
    assert res.n_imaginary.tolist() == [1]
    f = res.frequencies(0).cpu().numpy()
    assert f[0] < 0 and (f[1:] > 0).all() and _rel(f, ref["freq_wavenumber"]) <= 1e-10
    out = _vib().thermo(res, torch.zeros(1, dtype=torch.float64, device=DEV))
    want = vo.rrho(ref, 0.0)
    assert out["n_imaginary"].tolist() == [1] and abs(out["zpe"].item() / want["zpe"] - 1) <= 1e-10      # the imaginary mode is left out


def test_f32_hessians_match_their_widened_copy_bit_for_bit():
    graphs = _batch()
    a = _analyse(graphs, torch.float32)
    H, pos, mass = _device_inputs(graphs, torch.float32)
    b = _vib().harmonic_analysis([h.double() for h in H], pos, mass, **UNITS)
    for name in ("eigenvalue", "freq_wavenumber", "vib_temperature", "reduced_mass", "force_const", "norm_mode", "sigma", "moments", "sweeps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_a_graph_has_the_same_bits_alone_in_the_batch_and_in_the_reversed_batch():
    graphs = _batch()[:8]                          # the graphs that take the kernel
    one, two, rev = _analyse(graphs), _analyse(graphs), _analyse(graphs[::-1])
    names = ("eigenvalue", "freq_wavenumber", "vib_temperature", "reduced_mass", "force_const", "norm_mode")
    for name in names + ("sweeps", "sigma", "moments", "n_tr"):
        assert torch.equal(getattr(one, name), getattr(two, name)), name             # two runs are identical
    for g in range(len(graphs)):
        alone, r = _analyse(graphs[g : g + 1]), len(graphs) - 1 - g
        for other, h in ((one, g), (rev, r)):
            assert torch.equal(alone.eigenvalues(0), other.eigenvalues(h)) and torch.equal(alone.modes(0), other.modes(h)), g
            assert torch.equal(alone.frequencies(0), other.frequencies(h)) and torch.equal(alone.reduced_mass, other.reduced_mass[other._rows(h)]), g
            assert alone.sweeps[0].item() == other.sweeps[h].item() and alone.sigma[0].item() == other.sigma[h].item(), g


def test_a_periodic_cell_loses_three_modes():
    pos, mass = vo.molecule(8, 31)
    H = vo.synthetic_hessian(pos, mass, 32)
    ref = vo.harmonic(H, pos, mass, periodic=True)
    res = _analyse(((pos, mass, H, ref),), periodic=True)
    assert res.periodic and res.n_tr.tolist() == [3] == [ref["n_tr"]] and res.eigenvalues(0).numel() == 21
    lam = res.eigenvalues(0).cpu().numpy()
    e_val = np.abs(lam - ref["eigenvalue"]).max() / (24 * U52 * np.abs(ref["eigenvalue"]).max())
    print(f"vib periodic 8 atoms: |dlambda| {e_val:.3f} of 24 2^-52 max|lambda|")
    assert e_val <= 4 and _rel(res.frequencies(0).cpu().numpy(), ref["freq_wavenumber"]) <= 1e-10
    with pytest.raises(ValueError, match="periodic"):
        _vib().thermo(res, torch.zeros(1, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("T", [298.15, 1000.0])
def test_thermo_against_the_oracle(T):
    graphs = _batch()
    res = _analyse(graphs)
    energies = -10.0 - np.arange(len(graphs)) * 1.37
    first = lib.launch_count()
    out = _vib().thermo(res, torch.tensor(energies, device=DEV), temperature_K=T, symmetry_number=2, multiplicity=3)
    assert lib.launch_names(first) == ["xeq_vib_thermo_sums"]
    worst = 0.0
    for g, (_, _, _, ref) in enumerate(graphs):
        want = vo.rrho(ref, energies[g], T=T, symmetry_number=2, multiplicity=3)
        for key, w in want.items():
            got = out[key][g].item()
            err = abs(got - w) / abs(w) if w != 0 else abs(got)
            worst = max(worst, err)
            assert err <= 1e-10, (g, key, got, w)
    print(f"vib thermo T={T}: worst relative difference {worst:.2e}")
    per_graph = _vib().thermo(res, torch.tensor(energies, device=DEV), temperature_K=T, symmetry_number=torch.full((len(graphs),), 2.0), multiplicity=3)
    assert torch.equal(per_graph["g_tot"], out["g_tot"])


# ------------------------------------------------------------------------------------------------------------ the public entry on a model
def test_vibrations_on_a_small_model():
    import copy

    from tests import hessian_cases as hc
    from xequinet_amd import hessian as hz

    vib = _vib()
    pos = np.array([[0.0, 0.0, 0.1], [0.76, 0.0, -0.48], [-0.74, 0.05, -0.5],
                    [6.0, 0.0, 0.0], [6.63, 0.63, 0.63], [5.37, -0.63, 0.63], [5.37, 0.63, -0.63], [6.63, -0.63, -0.6]])
    z = np.array([8, 1, 1, 6, 1, 1, 1, 1])
    amu = {1: 1.008, 6: 12.011, 8: 15.999}
    host = hc.host_batch(pos, z, [0, 3, 8])
    data = hc.to_device(host, torch.float64)
    masses = torch.tensor([amu[int(v)] for v in z], dtype=torch.float64, device=DEV)
    model = copy.deepcopy(hc.model_case("well")[0]).to(torch.float64).to(DEV).eval().requires_grad_(False)
    blocks = hz.hessian(model, data, symmetrize=True)
    first = lib.launch_count()
    direct = vib.harmonic_analysis(blocks, data["pos"], masses, data["ptr"], **UNITS)
    assert lib.launch_names(first) == ["xeq_vib_project", "xeq_vib_eigh", "xeq_vib_finish"]
    first = lib.launch_count()
    vib.thermo(direct, torch.zeros(2, dtype=torch.float64, device=DEV))
    assert lib.launch_count() - first == 1
    whole = vib.vibrations(model, data, masses, **UNITS)
    assert not whole.periodic and whole.n_tr.tolist() == [6, 6] and whole.solver == ["kernel", "kernel"]
    for name in ("eigenvalue", "freq_wavenumber", "vib_temperature", "reduced_mass", "force_const", "norm_mode", "sigma", "moments", "sweeps"):
        assert torch.equal(getattr(whole, name), getattr(direct, name)), name
    for g, (a, b) in enumerate(((0, 3), (3, 8))):
        m = 3 * (b - a)
        ref = vo.harmonic(blocks[g].cpu().numpy(), pos[a:b], masses[a:b].cpu().numpy())
        lam = direct.eigenvalues(g).cpu().numpy()
        top = np.abs(ref["eigenvalue"]).max()
        bound = 4 * m * U52 * top
        e_val = np.abs(lam - ref["eigenvalue"]).max()
        print(f"vib model graph {g}: |dlambda| {e_val / (m * U52 * top):.3f} of m 2^-52 max|lambda|, wavenumbers {direct.frequencies(g).cpu().numpy().round(1).tolist()}")
        assert lam.shape == (m - 6,) and e_val <= bound
        # d sqrt(l) / sqrt(l) = dl / 2 l: the eigenvalue bound carried to each wavenumber, and 1e-10 for the arithmetic behind it
        tol = 1e-10 + bound / np.abs(ref["eigenvalue"])
        assert (np.abs(direct.frequencies(g).cpu().numpy() - ref["freq_wavenumber"]) <= tol * np.abs(ref["freq_wavenumber"])).all()
        assert direct.n_imaginary[g].item() == ref["n_imaginary"]
