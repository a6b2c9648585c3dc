"""Host side of the canonical thermostats (md.Dynamics ensembles "nose_hoover" and "bussi"): the record and the
constants against the header, the constructor's argument checks, and the oracle of tests/nvt_oracle.py itself -- that its chain conserves
what it should at second order, that its Bussi step samples the canonical kinetic-energy distribution, that no accept decision of the
gamma sampler the GPU tests meet is close enough for a device library's last bits to flip it, and that the chi-square draws the GPU
moment test compares keep the bound that test applies."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import md_oracle as mo
from tests import nvt_oracle as no

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "xeq.h")
ACCEL, KB = 9.648533212331002e-3, 8.617333262145179e-5       # eV, Angstrom (tests/test_md_host.py checks the package's against these)
T_K = 300.0


def _header() -> str:
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


# ------------------------------------------------------------------------------------------------------------------ 1. interface
def test_the_record_and_the_constants_are_the_headers():
    from xequinet_amd import lib

    text = _header()
    body = re.search(r"struct\s+xeq_nvt_params\s*\{(.*?)\}\s*;", text, flags=re.S).group(1)
    assert re.search(r"typedef\s+struct\s+xeq_nvt_params\s+xeq_nvt_params\s*;", text)
    members = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, decl
        members.append((m.group(3), bool(m.group(2)), m.group(1)))
    rec = lib.NvtParams
    assert rec.__name__ == "xeq_nvt_params" and [f[0] for f in rec._fields_] == [m[0] for m in members]
    for (name, kind), (_, pointer, base) in zip(rec._fields_, members):
        want = ctypes.c_void_p if pointer else {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}[base]
        assert kind is want, name
    const = {k: int(v) for k, v in re.findall(r"^#define\s+(XEQ_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    for enum in re.findall(r"enum\s*\{(.*?)\}", text, flags=re.S):
        const.update({k: int(v) for k, v in re.findall(r"(XEQ_\w+)\s*=\s*(-?\d+)", enum)})
    names = [k for k in const if k.startswith("XEQ_NVT_")]
    assert set(names) == {"XEQ_NVT_ROW", "XEQ_NVT_MAX_CHAIN", "XEQ_NVT_GAMMA_TRIES", "XEQ_NVT_PURPOSE", "XEQ_NVT_SCALE", "XEQ_NVT_BATH", "XEQ_NVT_XI",
                          "XEQ_NVT_VXI", "XEQ_NVT_NOSE_HOOVER", "XEQ_NVT_BUSSI"}
    for k in names:
        assert getattr(lib, k[len("XEQ_"):]) == const[k], k
    assert lib.REC_NVT == const["XEQ_REC_NVT"] and lib.REC_NVT >= len(lib.RECORDS) and lib.RECORDS_APART == {lib.REC_NVT: rec}
    assert const["XEQ_NVT_VXI"] + const["XEQ_NVT_MAX_CHAIN"] == const["XEQ_NVT_ROW"] and const["XEQ_NVT_XI"] + const["XEQ_NVT_MAX_CHAIN"] == const["XEQ_NVT_VXI"]
    assert const["XEQ_NVT_PURPOSE"] not in (const["XEQ_MD_PURPOSE_LANGEVIN"], const["XEQ_MD_PURPOSE_MAXWELL"]) and 0 <= const["XEQ_NVT_PURPOSE"] < 4
    # the oracle restates the same numbers
    assert (no.ROW, no.MAX_CHAIN, no.TRIES, no.PURPOSE, no.SCALE, no.BATH, no.XI, no.VXI, no.NOSE_HOOVER, no.BUSSI) == tuple(
        const["XEQ_NVT_" + k] for k in ("ROW", "MAX_CHAIN", "GAMMA_TRIES", "PURPOSE", "SCALE", "BATH", "XI", "VXI", "NOSE_HOOVER", "BUSSI"))
    L = lib.load()
    assert ctypes.sizeof(rec) == 8 * len(members) == L.xeq_record_bytes(lib.REC_NVT)
    assert "xeq_nvt_front" in lib.EXPORTS and "xeq_nvt_back" in lib.EXPORTS
    R = ctypes.POINTER
    assert L.xeq_nvt_front.argtypes[:3] == [R(lib.ResSystem), R(lib.MdParams), R(rec)]
    assert L.xeq_nvt_back.argtypes[:6] == [R(lib.ResSystem), R(lib.ResStep), R(lib.ResChunks), R(lib.MdParams), R(rec), R(lib.ResRecorder)]
    for name in ("xeq_nvt_front", "xeq_nvt_back"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name


def test_the_entries_refuse_a_wrong_record_before_any_launch():
    from xequinet_amd import lib

    L = lib.load()
    system = lib.fill(lib.ResSystem(), dtype=1, n=0, n_graphs=0, n_chunks=0)
    md_rec, step, chunks = lib.MdParams(), lib.ResStep(), lib.ResChunks()
    for bad, word in ((dict(kind=2, kT=1.0, tau=1.0), "thermostat 2"), (dict(kind=0, chain_length=9, kT=1.0, tau=1.0), "chain length 9"),
                      (dict(kind=0, chain_length=0, kT=1.0, tau=1.0), "chain length 0"), (dict(kind=1, kT=0.0, tau=1.0), "k_B T"),
                      (dict(kind=1, kT=1.0, tau=float("nan")), "tau")):
        nvt = lib.fill(lib.NvtParams(), **bad)
        assert L.xeq_nvt_front(ctypes.byref(system), ctypes.byref(md_rec), ctypes.byref(nvt), 0.5, None) != 0
        assert word in L.xeq_last_error().decode(), (bad, L.xeq_last_error().decode())
        assert L.xeq_nvt_back(ctypes.byref(system), ctypes.byref(step), ctypes.byref(chunks), ctypes.byref(md_rec), ctypes.byref(nvt), None, 1, None) != 0
    assert L.xeq_nvt_front(ctypes.byref(system), ctypes.byref(md_rec), None, 0.5, None) != 0 and "null argument record" in L.xeq_last_error().decode()


def test_the_ensembles_and_the_constructors_argument_checks():
    from xequinet_amd import lib, md

    assert md.THERMOSTATS == {"nose_hoover": lib.NVT_NOSE_HOOVER, "bussi": lib.NVT_BUSSI}
    assert not set(md.THERMOSTATS) & set(md.ENSEMBLES)            # ENSEMBLES stays the map to xeq_md_front's codes

    def make(**kw):          # every refusal below comes before the model or a device is looked at
        return md.Dynamics(None, torch.zeros(3, 3), torch.ones(3, dtype=torch.int64), torch.ones(3), timestep_fs=0.5, **kw)

    with pytest.raises(ValueError, match="'bussi'.*'nose_hoover'"):
        make(ensemble="andersen")
    for ens in ("nose_hoover", "bussi"):
        with pytest.raises(ValueError, match="temperature_K"):
            make(ensemble=ens, taut_fs=20.0)
        with pytest.raises(ValueError, match="temperature_K"):
            make(ensemble=ens, temperature_K=0.0, taut_fs=20.0)
        with pytest.raises(ValueError, match="taut_fs"):
            make(ensemble=ens, temperature_K=T_K)
        with pytest.raises(ValueError, match="taut_fs"):
            make(ensemble=ens, temperature_K=T_K, taut_fs=0.0)
        with pytest.raises(ValueError, match="npt_berendsen"):
            make(ensemble=ens, temperature_K=T_K, taut_fs=20.0, pressure_GPa=0.0)
    for n in (0, 9, 2.5):
        with pytest.raises(ValueError, match="chain_length"):
            make(ensemble="nose_hoover", temperature_K=T_K, taut_fs=20.0, chain_length=n)
    for ens in ("bussi", "berendsen", "nve"):
        with pytest.raises(ValueError, match="chain_length belongs to ensemble 'nose_hoover'"):
            make(ensemble=ens, temperature_K=T_K, taut_fs=20.0, chain_length=3)
    for ens in ("nose_hoover", "langevin"):
        with pytest.raises(ValueError, match="graph_rng_id belongs to ensemble 'bussi'"):
            make(ensemble=ens, temperature_K=T_K, taut_fs=20.0, friction_per_fs=0.01, graph_rng_id=torch.zeros(1, dtype=torch.int64))


def test_the_integer_philox_is_md_oracles():
    for seed, gid, j, step in ((0, 0, 0, 0), (0x9E3779B97F4A7C15, 5 << 32, 3, 2**32 + 5), (11, 1099 << 32, 16, 7)):
        c = np.array([(gid | j) & no.MASK, (gid | j) >> 32, step & no.MASK, ((step >> 32) & no.MASK) | (no.PURPOSE << 30)], dtype=np.uint64)
        want = mo.philox4x32_10(c, np.array([seed & no.MASK, seed >> 32], dtype=np.uint64))
        got = no.philox_ints([int(v) for v in c], seed & no.MASK, seed >> 32)
        assert [int(v) for v in want] == list(got)
        z = mo.box_muller(want.reshape(1, 4))[0]
        z0, z1, u = no.block(seed, gid, j, step)
        assert abs(z0 - z[0]) <= 1e-13 and abs(z1 - z[1]) <= 1e-13 and u == (float(want[2]) + 1.0) * 2.0**-32


# ------------------------------------------------------------------------------------------------------------------ 2. the oracle's physics
SPRING, MASS_AMU, TAU_FS, DT_FS = 5.0, 12.011, 20.0, 0.5       # eV / A^2, g / mol, fs, fs: omega = sqrt(k A / m) = 0.0634 / fs, omega dt = 0.032


def _harmonic(n):
    """n atoms, each on a spring to its own site (one graph, open boundaries), velocities drawn at T_K by the host generator."""
    sites = np.stack(np.meshgrid(*[np.arange(4) * 2.0] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    masses = np.full(n, MASS_AMU)
    v0 = np.sqrt(KB * T_K * ACCEL / masses)[:, None] * mo.normals(7, 1, 0, np.arange(n, dtype=np.int64))

    def evaluate(x):
        d = np.asarray(x, dtype=np.float64) - sites
        return np.array([0.5 * SPRING * float((d * d).sum())]), -SPRING * d

    return sites, masses, v0, evaluate


def _run(n, ensemble, dt, n_steps, keep, **kw):
    sites, masses, v0, evaluate = _harmonic(n)
    return no.integrate(None, sites, np.full(n, 6), np.array([0, n]), masses, dt=dt, n_steps=n_steps, ensemble=ensemble, accel=ACCEL, kB=KB,
                        temperature=T_K, taut=TAU_FS, v0=v0, evaluate=evaluate, keep=keep, **kw)


@pytest.mark.parametrize("n", [3, 64])
def test_the_chains_conserved_energy_is_second_order(n):
    """20 000 steps of dt and the same time span at dt / 2: the band of epot + ekin + bath shrinks by at least 3 (second order gives 4).
    That it IS a conserved quantity: its band is at most a twentieth of the band of epot + ekin, the energy the thermostat moves in
    and out of the system over the same run."""
    bands, moved = [], []
    for halvings in (0, 1):
        out = _run(n, "nose_hoover", DT_FS / 2**halvings, 20000 * 2**halvings, ("epot", "ekin", "bath"), chain_length=3)
        h = np.array(out["epot"])[:, 0] + np.array(out["ekin"])[:, 0] + np.array(out["bath"])[:, 0]
        assert np.isfinite(h).all()
        bands.append(float(h.max() - h.min()))
        system = np.array(out["epot"])[:, 0] + np.array(out["ekin"])[:, 0]
        moved.append(float(system.max() - system.min()))
        t = np.array(out["ekin"])[:, 0] * 2.0 / (3 * n * KB)
        assert 0.25 * T_K < t[len(t) // 2 :].mean() < 4.0 * T_K            # (it is a thermostat: the temperature stays at its target's scale)
    print(f"nvt host: chain n={n}: conserved-energy band {bands[0]:.3e} at dt, {bands[1]:.3e} at dt/2 (ratio {bands[0] / bands[1]:.2f}); "
          f"epot + ekin moved by {moved[0]:.3e}")
    assert bands[0] <= 0.05 * moved[0]
    assert 3.0 * bands[1] <= bands[0]


def _tau_int(y):
    """Integrated autocorrelation time 1 + 2 sum rho of a series, with Sokal's automatic window (the first M with M >= 5 tau(M))."""
    y = np.asarray(y, dtype=np.float64) - np.mean(y)
    n = len(y)
    f = np.fft.rfft(y, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    rho = acf / acf[0]
    tau = 2.0 * np.cumsum(rho) - 1.0
    window = np.arange(n) >= 5.0 * tau
    m = int(np.argmax(window)) if window.any() else n - 1
    return max(float(tau[m]), 1.0)


@pytest.mark.parametrize("n", [3, 64])
def test_bussi_samples_the_canonical_kinetic_energy(n):
    """200 000 steps: mean Nf kT / 2 and variance Nf (kT)^2 / 2, each within 5 standard errors from the series' own integrated
    autocorrelation time."""
    steps = 200000
    out = _run(n, "bussi", DT_FS, steps, ("ekin",), seed=3)
    k = np.array(out["ekin"])[1000:, 0]                       # (the start is at the target already; 50 coupling times are dropped all the same)
    nf, kT = 3 * n, KB * T_K
    mean, var = float(k.mean()), float(k.var())
    dev2 = (k - mean) ** 2
    tau_k, tau_v = _tau_int(k), _tau_int(dev2)
    se_mean, se_var = math.sqrt(var * tau_k / len(k)), math.sqrt(float(dev2.var()) * tau_v / len(k))
    print(f"nvt host: bussi n={n}: integrated autocorrelation time {tau_k:.1f} steps (K), {tau_v:.1f} steps ((K - mean)^2); "
          f"mean {mean:.5e} (want {0.5 * nf * kT:.5e}, s.e. {se_mean:.2e}), variance {var:.5e} (want {0.5 * nf * kT * kT:.5e}, s.e. {se_var:.2e})")
    assert abs(mean - 0.5 * nf * kT) <= 5.0 * se_mean
    assert abs(var - 0.5 * nf * kT * kT) <= 5.0 * se_var


# ------------------------------------------------------------------------------------------------------------------ 3. accept margins
def test_no_accept_decision_of_the_gpu_tests_is_within_reach_of_a_librarys_last_bits():
    """Every (seed, graph id, step, Nf) a Bussi step of tests/test_gpu_nvt.py meets: |log u - rhs| >= 1e-9 at every attempt, and none
    runs into the fallback behind the 16th."""
    closest, most, count = math.inf, 0, 0
    for seed, gid, step, nf in no.gpu_draw_cases():
        trace = []
        no.chi_square(nf, seed, gid, step, trace)
        accepted = trace[-1][3] > 0.0 and trace[-1][1] < trace[-1][2]
        assert accepted, (seed, gid, step, nf)
        for j, log_u, rhs, v in trace:
            if v > 0.0:
                closest = min(closest, abs(log_u - rhs))
            else:
                assert abs(v) >= 1e-9, (seed, gid, step, nf, j)          # (the sign of v decides too)
        most, count = max(most, len(trace)), count + 1
    print(f"nvt host: {count} gamma draws of the GPU tests: closest accept margin {closest:.3e}, most attempts {most}")
    assert count > 3 * no.MOMENT_GRAPHS and closest >= 1e-9 and most < no.TRIES


# ------------------------------------------------------------------------------------------------------------------ 4. moments
@pytest.mark.parametrize("nf", no.MOMENT_NF)
def test_the_oracles_chi_square_draws_keep_the_gpu_moment_bound(nf):
    draws = np.array([no.chi_square(nf, no.MOMENT_SEED, g << 32, no.MOMENT_STEP)[1] for g in range(no.MOMENT_GRAPHS)])
    bound = 5.0 * math.sqrt(2.0 * (nf - 1) / no.MOMENT_GRAPHS)
    print(f"nvt host: chi-square Nf={nf}: mean {draws.mean():.4f} (want {nf - 1}, bound {bound:.4f}), variance {draws.var():.3f} (want {2 * (nf - 1)})")
    assert np.all(draws > 0.0) and abs(draws.mean() - (nf - 1)) <= bound
