"""Host side of the eigensolver above the LDS cap (xeq_vib_eigh_large): its numpy restatement (tests/vib_large_oracle.py) against
numpy.linalg, the C ABI's entry and the front's new keyword.  No GPU needed.

Bounds: the project's own (tests/test_gpu_vib.py): 4 m 2^-52 max|lambda| for eigenvalues and residuals, 4 m 2^-52 for V^T V - I, the
backward-error form m u |M| with a factor 4.  A plain numpy Householder + QL needed 0.02-0.15, 0.01-0.05 and 0.06-0.14 of the unit
m 2^-52 [max|lambda|] on these matrices, 1.4-2.1 iterations per eigenvalue on average and at most 7 for one; the ratios are printed
before they are asserted."""
import os

import numpy as np
import pytest
import torch

from tests import vib_large_oracle as lo
from tests import vib_oracle as vo

U52 = 2.0 ** -52


def spectra(m, rng):
    """The three families of tests/test_gpu_vib.py::_spectra (same draws, same order) and "shifted": m - 6 values in (-1, 1) below a
    six-fold top eigenvalue, the shape of M = P S P + sigma Q Q^T."""
    out = {"separated": np.arange(1, m + 1) - m / 3.0, "six decades": 10.0 ** rng.uniform(-6.0, 0.0, m),
           "repeated": np.repeat(np.arange(1, m // 3 + 2), 3)[:m].astype(float)}
    low = rng.uniform(-1.0, 1.0, m - 6)
    out["shifted"] = np.concatenate([low, np.full(6, 2.0 * np.linalg.norm(low))])       # sigma = 2 |P S P|_F
    return out


def matrices(m):
    """(name, symmetric matrix) per family, seed 100 + m."""
    rng = np.random.default_rng(100 + m)
    out = []
    for name, lam in spectra(m, rng).items():
        U = np.linalg.qr(rng.standard_normal((m, m)))[0]
        A = (U * lam) @ U.T
        out.append((name, 0.5 * (A + A.T)))
    return out


def ratios(A, w, Vt):
    """(|dlambda|, residual, orthogonality) in units of m 2^-52 [max|lambda|]."""
    m = A.shape[0]
    ref = np.linalg.eigvalsh(A)
    top = np.abs(ref).max()
    return (np.abs(w - ref).max() / (m * U52 * top), np.abs(A @ Vt.T - Vt.T * w).max() / (m * U52 * top),
            np.abs(Vt @ Vt.T - np.eye(m)).max() / (m * U52))


@pytest.mark.parametrize("m", [97, 257, 384])
def test_the_restatement_against_numpy(m):
    for name, A in matrices(m):
        w, Vt, iters, status = lo.eigh(A)
        e_val, e_res, e_orth = ratios(A, w, Vt)
        print(f"vib_large oracle m={m:3d} {name:11s}: iterations mean {np.mean(iters):.2f} max {max(iters)}, |dlambda| {e_val:.3f}, residual {e_res:.3f}, "
              f"orthogonality {e_orth:.3f}  (units of m 2^-52 [max|lambda|])")
        assert status == 0 and len(iters) == m and 1 <= max(iters) <= 30
        assert (np.diff(w) >= 0).all()
        assert e_val <= 4 and e_res <= 4 and e_orth <= 4
        lead = np.abs(Vt).argmax(axis=1)
        assert (Vt[np.arange(m), lead] > 0).all()


def test_the_restatement_on_structured_matrices():
    m = 12
    w, Vt, iters, status = lo.eigh(np.diag(np.arange(m, 0, -1.0)))
    assert status == 0 and max(iters) == 0 and (w == np.arange(1, m + 1.0)).all() and (Vt == np.eye(m)[::-1]).all()
    w, Vt, iters, status = lo.eigh(np.eye(m))
    assert status == 0 and max(iters) == 0 and (w == 1).all() and (Vt == np.eye(m)).all()
    w, Vt, iters, status = lo.eigh(np.array([[3.0]]))
    assert status == 0 and iters == [0] and w.tolist() == [3.0] and Vt.tolist() == [[1.0]]
    T = np.diag(np.arange(1.0, m + 1)) + np.diag(np.full(m - 1, 0.5), 1) + np.diag(np.full(m - 1, 0.5), -1)
    d, e, Qt = lo.tridiagonalise(T)
    assert (Qt == np.eye(m)).all() and (d == np.diag(T)).all() and (e[:-1] == 0.5).all()      # every Householder vector vanishes
    bad = np.eye(m)
    bad[3, 5] = bad[5, 3] = np.nan
    assert lo.eigh(bad)[3] == 1                                                              # and the loops end


def test_the_c_abi_exports_and_refuses():
    from xequinet_amd import lib

    assert "xeq_vib_eigh_large" in lib.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xeq.h")).read()
    assert "int xeq_vib_eigh_large(" in header and f"#define XEQ_VIB_LARGE_MAX_DIM {lib.VIB_LARGE_MAX_DIM}\n" in header
    assert lib.VIB_LARGE_MAX_DIM == 768 and f"#define XEQ_VIB_MAX_DIM {lib.VIB_MAX_DIM}\n" in header and lib.VIB_MAX_DIM == 96
    handle = lib.load()
    one, first = 8, lib.launch_count()
    rc = handle.xeq_vib_eigh_large(one, one, one, one, 1, lib.VIB_LARGE_MAX_DIM + 1, one, one, one, one, None)
    assert rc == 1 and b"XEQ_VIB_LARGE_MAX_DIM" in handle.xeq_last_error()
    assert handle.xeq_vib_eigh_large(None, None, None, None, 1, 99, None, None, None, None, None) == 1
    assert handle.xeq_vib_eigh_large(None, None, None, None, 0, 99, None, None, None, None, None) == 0       # nothing to do: no launch
    assert lib.launch_count() == first


def test_an_unknown_large_solver_is_refused():
    from xequinet_amd import vibrations as vib

    pos, mass = vo.molecule(3, 1)
    H = [torch.tensor(vo.synthetic_hessian(pos, mass, 2))]
    kw = dict(energy_unit="eV", length_unit="Angstrom")
    with pytest.raises(ValueError, match="large"):
        vib.harmonic_analysis(H, torch.tensor(pos), torch.tensor(mass), large="blocked", **kw)
    for large in ("tensor", "kernel"):                       # both are known: the next refusal is the host tensors'
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            vib.harmonic_analysis(H, torch.tensor(pos), torch.tensor(mass), large=large, **kw)
