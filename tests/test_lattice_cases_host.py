"""tests/lattice_cases.py on the CPU: the exact integer oracle equals the project's floating-point oracles in f32 AND in f64 on every
case (the condition under which the GPU tests may compare with exact equality and exclude no pair), the cases hold the ties they
were built for, and the exact lists are symmetric."""
import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests import lattice_cases as lc

FLOAT_ORACLE_MAX_ATOMS = 1024      # the periodic floating-point oracle holds all (center, neighbor, image) at once


def bins_of(case):
    """(rep, bins [G, 3]) as the periodic front computes them (data/radius_graph.py: _image_counts, _with_bins), on the CPU"""
    from xequinet_amd.data.radius_graph import _image_counts, _with_bins

    reps, prune = _image_counts(torch.tensor(lc.cells(case, np.float32)), case.pbc, case.rc, with_prune=True)
    return reps, _with_bins(prune, case.pbc)[3].numpy()


@pytest.mark.parametrize("name", lc.names())
def test_exact_oracle_equals_the_float_oracles_in_f32_and_f64(name):
    """Edges, offsets and order.  A case that fails here is not dyadic.  ``batch`` (1 089 atoms, 125 images) is beyond the float
    oracle's memory: its graphs are the cases sc8 and sc32_unwrapped, checked here on their own, and a lone atom."""
    c = lc.case(name)
    ei, off, ties = lc.exact(name)
    print(f"{name}: {c.n_atoms} atoms, {ei.shape[1]} edges, {ties} (i, j, image) on the cutoff = {ties / c.n_atoms:.2f} per atom")
    if c.periodic and c.n_atoms > FLOAT_ORACLE_MAX_ATOMS:
        assert name == "batch"
        return
    for dt in (np.float32, np.float64):
        pos = lc.positions(c, dt)
        assert np.array_equal(pos.astype(np.float64) * lc.UNIT, c.P8)                  # the cast lost nothing
        if c.periodic:
            want_ei, want_off = orc.radius_graph_pbc_oracle(pos, np.diff(c.ptr), c.pbc, lc.cells(c, dt), c.rc)
            np.testing.assert_array_equal(want_ei, ei, err_msg=f"{name} {dt.__name__}")
            np.testing.assert_array_equal(want_off, off.astype(dt), err_msg=f"{name} {dt.__name__}")
        else:
            np.testing.assert_array_equal(orc.radius_graph_canonical(pos, c.ptr, c.rc), ei, err_msg=f"{name} {dt.__name__}")
    assert ei.shape[1] > 0


@pytest.mark.parametrize("name", lc.names(periodic=True))
def test_every_periodic_case_has_lattice_vectors_exactly_on_the_cutoff(name):
    """Crystals: 30 per atom ((6,0,0) x 6, (4,4,2) x 24) where all three axes are periodic and the cell is full; the gases by chance
    of the 1/8 A grid (36 x 64 = 2 304 is a sum of three squares in many ways)."""
    c = lc.case(name)
    ties = lc.exact(name)[2]
    print(f"{name}: {ties} on the cutoff, {ties / c.n_atoms:.2f} per atom")
    assert ties > 0
    if name in ("sc8", "sc16", "sc32_faces", "sc32_unwrapped", "shear_xy", "shear_xy_yz", "small444", "small4816"):
        assert ties == 30 * c.n_atoms


@pytest.mark.parametrize("name", lc.names(periodic=False))
def test_open_cases_hold_their_ties_and_coincident_atoms(name):
    c = lc.case(name)
    ei, _, ties = lc.exact(name)
    print(f"{name}: {ei.shape[1]} edges, {ties} pairs on the cutoff")
    if name == "open_point":
        assert ei.shape[1] == 70 * 69 and ties == 0          # all at one place: everybody is everybody's neighbour, no distance but 0
    elif name.startswith("gas_coincident"):
        same = (c.P8[ei[0]] == c.P8[ei[1]]).all(1)
        assert int(same.sum()) == 60                          # coincident atoms ARE edges without a box
    else:
        assert ties > 0


def test_coincident_atoms_are_no_edges_with_a_box_and_an_eighth_apart_are():
    for name, want in (("gas_coincident", 0), ("gas_eighth", 60)):
        c = lc.case(name)
        ei, off, _ = lc.exact(name)
        d = c.P8[ei[0]] - c.P8[ei[1]] - np.einsum("ea,ab->eb", off, c.C8[0])
        d2 = (d * d).sum(1)
        assert int((d2 <= 1).sum()) == want and int(d2.min()) == (1 if want else d2.min())
        assert int(d2.max()) < (c.rc * lc.UNIT) ** 2


@pytest.mark.parametrize("name", lc.names())
def test_exact_list_is_symmetric(name):
    """(i, j, o) is present exactly when (j, i, -o) is; the numpy mirror map is an involution without a -1."""
    c = lc.case(name)
    ei, off, _ = lc.exact(name)
    off = np.zeros((ei.shape[1], 3), dtype=np.int64) if off is None else off
    rev = lc.mirror_map_np(ei, off, c.n_atoms)
    assert rev.min(initial=0) >= 0
    assert np.array_equal(rev[rev], np.arange(len(rev)))
    assert np.array_equal(ei[0][rev], ei[1]) and np.array_equal(off[rev], -off)
    assert bool((np.diff(ei[0]) >= 0).all())


def test_bin_counts_and_image_counts_of_the_cases():
    """What the cell-list form sees: one axis with five bins and two with two on the 32 x 16 x 16 cell (the wrapped b - 1 / b + 1 walk
    next to the visit-each-bin-once axes), five on every axis for the thin gas, one bin where the cell is smaller than the cutoff;
    two images per axis there, and for the whole batch that holds such a cell."""
    seen = {}
    for name in lc.names(periodic=True):
        c = lc.case(name)
        reps, nb = bins_of(c)
        assert reps == lc.n_images(c.C8, c.pbc, c.rc)
        seen[name] = (reps, nb.tolist())
        print(f"{name}: rep {reps}, bins {nb.tolist()}")
    assert seen["sc32_faces"][1] == [[5, 2, 2]] and seen["sc32_unwrapped"][1] == [[5, 2, 2]]
    assert seen["gas_bins555"][1] == [[5, 5, 5]]
    assert seen["small444"] == ([2, 2, 2], [[1, 1, 1]]) and seen["small4816"] == ([2, 1, 1], [[1, 1, 2]])
    assert seen["batch"] == ([2, 2, 2], [[1, 1, 1], [1, 1, 1], [1, 1, 1], [5, 2, 2]])
    assert seen["slab"] == ([1, 1, 0], [[2, 2, 1]]) and seen["wire"] == ([1, 0, 0], [[2, 1, 1]])


def test_single_system_lists_reach_every_neighbour():
    """xeq::radius_graph_pbc does not wrap: on positions inside the cell (faces included) its images still reach every neighbour, so
    the list has as many edges as the wrapped one."""
    for name in lc.SINGLE_SYSTEM:
        pw, ei, off = lc.exact_single_system(name)
        assert ei.shape[1] == lc.exact(name)[0].shape[1] and off.shape == (ei.shape[1], 3)


def _fcc_lists(variant, displaced=False):
    pos, _, _, cell = lc.fcc_shell(variant, displaced)
    e32, o32 = orc.radius_graph_pbc_oracle(pos, np.array([108]), [True] * 3, cell, lc.FCC_RC)
    e64, o64 = orc.radius_graph_pbc_oracle(pos.astype(np.float64), np.array([108]), [True] * 3, cell.astype(np.float64), lc.FCC_RC)
    missing = int((lc.mirror_map_np(e32, o32.astype(np.int64), 108) < 0).sum())
    return e32.shape[1], e64.shape[1], lc.list_differences(e32, o32, e64, o64), missing


def test_fcc_shell_sits_on_the_cutoff_in_rounding():
    """The f32 oracle's list of the FCC case is not the f64 oracle's on the same f32 numbers: at a = f32(5 / sqrt 2) f32 puts the whole
    fourth shell outside and f64 inside (1 296 = 12 x 108 edges differ, the f32 list is still symmetric); three ulps below, the shell
    splits and 45 edges of the f32 list have no mirror.  Both variants are kept (lc.FCC_VARIANTS).  With the atoms displaced the
    lists agree and are symmetric."""
    assert lc.fcc_shell()[0].shape == (108, 3) and lc.FCC_VARIANTS == (0, -3)
    for variant in lc.FCC_VARIANTS:
        n32, n64, diff, missing = _fcc_lists(variant)
        print(f"fcc_shell a{variant:+d}ulp: f32 list {n32} edges, f64 list {n64}, {diff} differ, {missing} of the f32 list have no mirror")
        assert 108 * 42 <= n32 <= 108 * 54 and 108 * 42 <= n64 <= 108 * 54 and diff > 0
        assert (missing > 0) == (variant == -3)
        n32, n64, diff, missing = _fcc_lists(variant, displaced=True)
        assert n32 == n64 and diff == 0 and missing == 0
