"""Host side of the harmonic analysis (xequinet_amd/vibrations.py): the numpy oracle of tests/vib_oracle.py against closed forms, the
front's refusals, the lazy attribute and the C ABI's entries.  No GPU needed.

Bounds: the closed forms and the oracle are two f64 evaluations of the same few operations on 6 x 6 / 9 x 9 matrices; 1e-10 relative
leaves four decades over their rounding (the rigid-body projection of a 9 x 9 matrix costs about 1e-15).  Sackur-Tetrode for argon is
compared with the tabulated standard molar entropy at 1 bar, 154.846 J / (mol K) (CODATA key values; argon has no other degree of
freedom), less R ln(1.01325) = 0.109 for 1 atm, to 0.01."""
import math

import numpy as np
import pytest
import torch

from tests import vib_oracle as vo


def _spring(pos, pairs, k):
    """Hessian [n, n, 3, 3] of sum k/2 (|r_i - r_j| - r0)^2 at its minimum: k e e^T on the pair's blocks."""
    n = len(pos)
    F = np.zeros((n, 3, n, 3))
    for i, j in pairs:
        e = (pos[i] - pos[j]) / np.linalg.norm(pos[i] - pos[j])
        B = k * np.outer(e, e)
        F[i, :, i, :] += B
        F[j, :, j, :] += B
        F[i, :, j, :] -= B
        F[j, :, i, :] -= B
    return F.transpose(0, 2, 1, 3)


def test_diatomic_frequency_is_sqrt_k_over_mu():
    m1, m2, k = 1.008, 34.969, 30.0                    # eV / Angstrom^2
    d = np.array([0.3, -0.5, 0.81])
    pos = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3] + 1.27 * d / np.linalg.norm(d)])
    res = vo.harmonic(_spring(pos, [(0, 1)], k), pos, np.array([m1, m2]))
    assert res["n_tr"] == 5 and res["rotor"] == vo.LINEAR and len(res["eigenvalue"]) == 1
    mu = m1 * m2 / (m1 + m2)
    want = math.sqrt(k * 1.602176634e-19 / (1e-20 * mu * 1.66053906660e-27)) / (2 * math.pi * 299792458.0 * 100.0)
    assert abs(res["freq_wavenumber"][0] / want - 1) <= 1e-10
    # pyscf's convention: 1 / sum (v_i^2 / m_i) of the unit mass-weighted vector v = (sqrt(mu / m1), -sqrt(mu / m2)) along the bond
    rm = 1.0 / (mu * (1 / m1 ** 2 + 1 / m2 ** 2))
    assert abs(res["reduced_mass"][0] / rm - 1) <= 1e-10 and abs(res["force_const"][0] / (rm * k / mu) - 1) <= 1e-10
    assert 2000 < want < 4000                           # an H-Cl-like stretch, in cm^-1


def test_symmetric_linear_triatomic_has_its_three_analytic_frequencies():
    mB, mA, k, kb = 15.999, 12.011, 100.0, 5.0
    pos = np.array([[-1.16, 0, 0], [0, 0, 0], [1.16, 0, 0]], dtype=float)
    H = _spring(pos, [(0, 1), (1, 2)], k)
    g = np.array([1.0, -2.0, 1.0])                      # the bend: kb / 2 (y0 - 2 y1 + y2)^2 for y and for z
    for a in (1, 2):
        H[:, :, a, a] += kb * np.outer(g, g)
    res = vo.harmonic(H, pos, np.array([mB, mA, mB]))
    assert res["n_tr"] == 5 and res["rotor"] == vo.LINEAR and len(res["eigenvalue"]) == 4
    bend, sym, asym = kb * (2 / mB + 4 / mA), k / mB, k * (1 / mB + 2 / mA)
    want = np.sort([bend, bend, sym, asym])
    assert np.abs(res["eigenvalue"] / want - 1).max() <= 1e-10
    assert abs(res["eigenvalue"][0] - res["eigenvalue"][1]) <= 1e-10 * bend         # the doubly degenerate bend
    assert np.abs(res["modes"].T @ res["q"]).max() <= 1e-12


def test_one_harmonic_mode_at_a_given_theta_over_t():
    T, x = 300.0, 1.7
    s = vo.thermo_sums(np.array([x * T]), np.array([1.0]), T)
    assert abs(s[0] - x * T / 2) <= 1e-12 * x * T
    assert abs(s[1] / T - x * (0.5 / math.tanh(x / 2) - 0.5)) <= 1e-12                                      # theta / (e^x - 1)
    assert abs(s[2] - (x / 2 / math.tanh(x / 2) - math.log(2 * math.sinh(x / 2)))) <= 1e-12                 # S_vib / k
    assert abs(s[3] - (x / 2) ** 2 / math.sinh(x / 2) ** 2) <= 1e-12                                        # Cv / k
    assert (vo.thermo_sums(np.array([500.0, 800.0]), np.array([-1.0, 1.0]), T) == vo.thermo_sums(np.array([800.0]), np.array([1.0]), T)).all()


def test_sackur_tetrode_for_argon():
    res = {"mass_tot": 39.948, "moments": np.zeros(3), "rotor": vo.ATOM, "vib_temperature": np.zeros(0), "eigenvalue": np.zeros(0)}
    out = vo.rrho(res, 0.0, T=298.15, P=101325.0, energy_unit="kJ/mol")
    R = vo.K_B * vo.N_A / 1000.0
    assert abs(out["s_trans"] * 1000.0 - (154.846 - 1000.0 * R * math.log(1.01325))) <= 0.01
    bar = vo.rrho(res, 0.0, T=298.15, P=100000.0, energy_unit="kJ/mol")
    assert abs(bar["s_trans"] * 1000.0 - 154.846) <= 0.01
    assert out["s_rot"] == 0.0 and out["s_vib"] == 0.0 and out["zpe"] == 0.0
    assert abs(out["cp_tot"] / R - 2.5) <= 1e-12 and abs(out["h_tot"] / (R * 298.15) - 2.5) <= 1e-12


def _host_case():
    pos, mass = vo.molecule(3, 1)
    H = torch.tensor(vo.synthetic_hessian(pos, mass, 2))
    return [H], torch.tensor(pos), torch.tensor(mass)


def test_refusals():
    from xequinet_amd import vibrations as vib

    H, pos, mass = _host_case()
    kw = dict(energy_unit="eV", length_unit="Angstrom")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vib.harmonic_analysis(H, pos, mass, **kw)
    with pytest.raises(ValueError, match="n, n, 3, 3"):
        vib.harmonic_analysis([H[0].reshape(9, 9)], pos, mass, **kw)
    with pytest.raises(ValueError, match="list of tensors"):
        vib.harmonic_analysis(H[0], pos, mass, **kw)
    with pytest.raises(ValueError, match="pos"):
        vib.harmonic_analysis(H, pos[:2], mass, **kw)
    with pytest.raises(ValueError, match="masses"):
        vib.harmonic_analysis(H, pos, mass[:2], **kw)
    with pytest.raises(ValueError, match="float64"):
        vib.harmonic_analysis(H, pos, mass.float(), **kw)
    with pytest.raises(ValueError, match="ptr"):
        vib.harmonic_analysis(H, pos, mass, [0, 2, 1], **kw)
    with pytest.raises(ValueError, match="ptr"):
        vib.harmonic_analysis(H, pos, mass, torch.tensor([0, 2]), **kw)
    with pytest.raises(ValueError, match="share one dtype"):
        vib.harmonic_analysis([H[0], H[0].float()], torch.cat([pos, pos]), torch.cat([mass, mass]), **kw)
    with pytest.raises(ValueError, match="Invalid unit"):
        vib.harmonic_analysis(H, pos, mass, energy_unit="furlong")


def test_a_missing_energy_unit_is_refused():
    from xequinet_amd import vibrations as vib
    from xequinet_amd.utils import units as U

    H, pos, mass = _host_case()
    saved = dict(U.DEFAULT_UNITS_MAP)
    try:
        U.DEFAULT_UNITS_MAP.clear()
        U.DEFAULT_UNITS_MAP.update({"pos": "Angstrom"})
        with pytest.raises(ValueError, match="energy unit"):
            vib.harmonic_analysis(H, pos, mass)
        U.set_default_units({"energy": "eV"})
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # the units are known now: the next refusal is the host tensors'
            vib.harmonic_analysis(H, pos, mass)
    finally:
        U.DEFAULT_UNITS_MAP.clear()
        U.DEFAULT_UNITS_MAP.update(saved)


def test_thermo_refuses_a_periodic_result_and_bad_arguments():
    from xequinet_amd import vibrations as vib

    z = torch.zeros(0, dtype=torch.float64)
    zi = torch.zeros(1, dtype=torch.int32)

    def result(periodic):
        return vib.HarmonicResult(eigenvalue=z, freq_wavenumber=z, vib_temperature=z, reduced_mass=z, force_const=z, norm_mode=z,
                                  mode_ptr=torch.zeros(2, dtype=torch.int64), ptr=[0, 1], n_tr=zi, rotor=zi, moments=torch.zeros((1, 3), dtype=torch.float64),
                                  mass_tot=torch.ones(1, dtype=torch.float64), n_imaginary=zi, sweeps=zi, status=zi, sigma=torch.ones(1, dtype=torch.float64),
                                  solver=["kernel"], periodic=periodic, energy_unit="eV", length_unit="Angstrom", mode_ptr_host=[0, 0], mode_off_host=[0, 0])

    e = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError, match="periodic"):
        vib.thermo(result(True), e)
    with pytest.raises(ValueError, match="temperature"):
        vib.thermo(result(False), e, temperature_K=0.0)
    with pytest.raises(ValueError, match="multiplicity"):
        vib.thermo(result(False), e, multiplicity=0)
    with pytest.raises(ValueError, match="energies"):
        vib.thermo(result(False), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vib.thermo(result(False), e)
    r = result(False)
    assert r.num_graphs == 1 and r.frequencies(0).numel() == 0 and tuple(r.modes(0).shape) == (0, 1, 3)


def test_unit_factors_agree_with_the_oracle_constants():
    from xequinet_amd import vibrations as vib

    f = vib.unit_factors("eV", "Angstrom")
    lam = np.array([2.5])
    om = vo.omega_si(lam)
    assert abs(f["to_wavenumber"] * math.sqrt(2.5) / (om[0] / (2 * math.pi * vo.C_LIGHT * 100.0)) - 1) <= 1e-14
    assert abs(f["to_kelvin"] * math.sqrt(2.5) / (om[0] * vo.H_PLANCK / (2 * math.pi * vo.K_B)) - 1) <= 1e-14
    g = vib.unit_factors("kcal/mol", "nm")
    assert abs(g["energy_J"] / vo.ENERGY_J["kcal/mol"] - 1) <= 1e-14 and abs(g["length_m"] / 1e-9 - 1) <= 1e-14


def test_the_package_exports_the_module_lazily():
    import xequinet_amd
    from xequinet_amd import vibrations as vib

    assert xequinet_amd.vibrations is vib
    assert callable(vib.harmonic_analysis) and callable(vib.thermo) and callable(vib.vibrations)


def test_the_c_abi_exports_and_refuses():
    from xequinet_amd import lib

    for name in ("xeq_vib_project", "xeq_vib_eigh", "xeq_vib_finish", "xeq_vib_thermo_sums"):
        assert name in lib.EXPORTS
    handle = lib.load()
    header = open(__file__.replace("tests/test_vib_host.py", "include/xeq.h")).read()
    assert f"#define XEQ_VIB_MAX_DIM {lib.VIB_MAX_DIM}\n" in header and f"#define XEQ_VIB_MAX_SWEEPS {lib.VIB_MAX_SWEEPS}\n" in header
    one, first = 8, lib.launch_count()
    rc = handle.xeq_vib_eigh(one, one, one, one, 1, lib.VIB_MAX_DIM + 1, one, one, one, one, None)
    assert rc == 1 and b"XEQ_VIB_MAX_DIM" in handle.xeq_last_error()
    assert handle.xeq_vib_eigh(None, None, None, None, 1, 9, None, None, None, None, None) == 1
    assert handle.xeq_vib_eigh(None, None, None, None, 0, 9, None, None, None, None, None) == 0            # nothing to do: no launch
    assert handle.xeq_vib_project(5, None, None, None, None, None, 1, 0, *([None] * 10), None) == 1        # bad dtype code
    assert handle.xeq_vib_thermo_sums(None, None, one, 1, 0.0, one, None) == 1 and b"temperature" in handle.xeq_last_error()
    assert handle.xeq_vib_finish(*([None] * 5), 0, *([None] * 3), 1.0, 1.0, *([None] * 7), None) == 0
    assert lib.launch_count() == first
    from xequinet_amd.csrc import build

    assert "xeq_vib.hip" in build.SOURCES and "xeq_vib.hip" not in build.MFMA_SOURCES
