"""Neighbour-list cases on which every correct evaluation agrees, and the exact integer oracle for them.  CPU only, numpy only; no test
functions here (tests/test_lattice_cases_host.py checks this module, tests/test_gpu_lattice_lists.py runs the builders of
csrc/xeq_graph.hip on it).

The list tests of tests/test_gpu_parity.py draw positions from continuous distributions: a pair exactly at the cutoff, an atom exactly
on a cell face or a bin edge, two atoms at one place and a whole shell of equal distances all have probability zero there, and a
crystal has all of them at once.  Here positions are integer multiples of 1/8 A (``P8``) and cells have small integer entries with a
DYADIC inverse (``C8``, the same unit), so every intermediate of the search -- fractional coordinates, their floor, wrapped positions,
image vectors, differences, squares (multiples of 1/64, far below 2^24 of them) and their sum -- is exactly representable in f32.  A
correctly rounded square root is monotone, so D < rc holds exactly when D^2 < rc^2 in integers, whatever the order of operations, fma
or not, f32 or f64: the truth is an integer computation and the comparison is exact equality with no pair excluded.

``exact_pbc_list`` / ``exact_open_list`` are that integer computation in the reference's order (center-major, then
neighbor * n_cells + cell ascending; data/radius_graph.py:177-181), in chunks of centers.  Each family below states its cutoff and
asserts that its own data is dyadic (``_assert_dyadic``).

The last section is the opposite case: an FCC crystal whose fourth shell sits on the cutoff only in real arithmetic (``fcc_shell``)."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import xpainn_oracle as orc

UNIT = 8                                   # positions and cells are integers in 1/UNIT A
UNWRAP8 = (-3 * UNIT, 1, 17 * UNIT)        # (-3, 0.125, 17) A: puts atoms below 0 and above 1 in fractional coordinates
_CHUNK_BYTES = 48 << 20


# ---------------------------------------------------------------------------------------------------------------- exact oracle
def _int_inverse(C):
    """adj, det of an integer 3 x 3 matrix with det > 0: inv(C) = adj / det"""
    C = np.asarray(C, dtype=np.int64)
    adj = np.empty((3, 3), dtype=np.int64)
    for r in range(3):
        for c in range(3):
            m = np.delete(np.delete(C, c, axis=0), r, axis=1)          # cofactor of (c, r): the adjugate is the transpose
            adj[r, c] = (-1) ** (r + c) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    det = int(C[0, 0] * adj[0, 0] + C[0, 1] * adj[1, 0] + C[0, 2] * adj[2, 0])
    assert det > 0, "right-handed cells only"
    return adj, det


def n_images(C8, pbc, rc):
    """images per axis, max over the batch: oracle._n_images on the cells in A (f64; no case sits within rounding of a whole number)"""
    return orc._n_images(np.asarray(C8, dtype=np.float64) / UNIT, pbc, float(rc))


def wrap_exact(P8, C8g, pbc):
    """(wrapped positions, shift) of one graph: shift = floor(P C^-1) on the periodic axes by integer floor division"""
    adj, det = _int_inverse(C8g)
    num = P8 @ adj                                        # fractional coordinates times det
    shift = np.zeros_like(P8)
    for ax in range(3):
        if pbc[ax]:
            shift[:, ax] = np.floor_divide(num[:, ax], det)
    return P8 - shift @ np.asarray(C8g, dtype=np.int64), shift


def _grid(reps):
    axes = [np.arange(-r, r + 1, dtype=np.int64) for r in reps]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)       # cartesian_prod order


def exact_pbc_list(P8, C8, pbc, rc, ptr=None, wrap=True, count_ties=False):
    """-> edge_index [2, E] int64, cell_offsets [E, 3] int64 (and, with ``count_ties``, the number of (i, j, image) exactly ON the
    cutoff).  P8 [N, 3] integer positions in 1/8 A, C8 [G, 3, 3] (or [3, 3]) integer cells in 1/8 A, ``ptr`` the graph pointer (one
    graph without it).  Pairs with 0 < D^2 < rc^2 (D > 0.01 is D > 0 on this grid), images -rep .. rep per axis.  ``wrap=False``: the
    single-system form (data/radius_graph.py:195-275), which searches the positions as given."""
    P8 = np.asarray(P8, dtype=np.int64)
    C8 = np.asarray(C8, dtype=np.int64).reshape(-1, 3, 3)
    ptr = np.array([0, len(P8)]) if ptr is None else np.asarray(ptr)
    assert len(C8) == len(ptr) - 1 and float(rc * UNIT).is_integer()
    r2 = int(rc * UNIT) ** 2
    offs = _grid(n_images(C8, pbc, rc))
    nc = len(offs)
    e0, e1, eo, ties = [], [], [], 0
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        n = b - a
        if n == 0:
            continue
        pw, shift = wrap_exact(P8[a:b], C8[g], pbc) if wrap else (P8[a:b], np.zeros((n, 3), dtype=np.int64))
        B = (pw[:, None, :] + (offs @ C8[g])[None, :, :]).reshape(-1, 3)         # atom-major, cell-minor
        chunk = max(1, _CHUNK_BYTES // (len(B) * 3 * 8))
        for s in range(0, n, chunk):
            d = pw[s:s + chunk, None, :] - B[None, :, :]
            d2 = (d * d).sum(-1)
            ix, iy = np.nonzero((d2 < r2) & (d2 > 0))
            ties += int((d2 == r2).sum())
            j = iy // nc
            e0.append(ix + s + a)
            e1.append(j + a)
            eo.append(offs[iy % nc] + (shift[ix + s] - shift[j]))
    if not e0:
        out = np.zeros((2, 0), dtype=np.int64), np.zeros((0, 3), dtype=np.int64)
    else:
        out = np.stack([np.concatenate(e0), np.concatenate(e1)]), np.concatenate(eo)
    return out + (ties,) if count_ties else out


def exact_open_list(P8, ptr, rc, count_ties=False):
    """-> edge_index [2, E] int64 sorted by (center, neighbor): same-graph pairs with D^2 < rc^2 and j != i (coincident atoms ARE
    edges without a box: cluster.radius_graph)."""
    P8 = np.asarray(P8, dtype=np.int64)
    assert float(rc * UNIT).is_integer()
    r2 = int(rc * UNIT) ** 2
    e0, e1, ties = [], [], 0
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        n = b - a
        if n == 0:
            continue
        p = P8[a:b]
        chunk = max(1, _CHUNK_BYTES // (n * 3 * 8))
        for s in range(0, n, chunk):
            d = p[s:s + chunk, None, :] - p[None, :, :]
            d2 = (d * d).sum(-1)
            m = d2 < r2
            m[np.arange(len(m)), np.arange(s, s + len(m))] = False
            ties += int((d2 == r2).sum())
            ix, iy = np.nonzero(m)
            e0.append(ix + s + a)
            e1.append(iy + a)
    ei = np.stack([np.concatenate(e0), np.concatenate(e1)]) if e0 else np.zeros((2, 0), dtype=np.int64)
    return (ei, ties) if count_ties else ei


def mirror_map_np(edge_index, cell_offsets, n_nodes):
    """position of (j, i, -o) for every edge (i, j, o) of a list, -1 where the list holds none"""
    o = np.asarray(cell_offsets, dtype=np.int64)
    R = 2 * int(np.abs(o).max(initial=0)) + 1

    def key(i, j, off):
        k = i * n_nodes + j
        for ax in range(3):
            k = k * R + (off[:, ax] + R // 2)
        return k

    k = key(edge_index[0], edge_index[1], o)
    order = np.argsort(k, kind="stable")
    want = key(edge_index[1], edge_index[0], -o)
    pos = np.searchsorted(k[order], want)
    pos = np.minimum(pos, len(k) - 1)
    hit = k[order][pos] == want if len(k) else np.zeros(0, dtype=bool)
    return np.where(hit, order[pos], -1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------ cases
def _assert_dyadic(P8, C8):
    """positions: integers in 1/8 A below 2^20 of them; cells: integer, right-handed, inverse with power-of-two denominators no
    finer than 2^-10, so that fractional coordinates (|P8| det-th parts) and everything after them fit 24 bits"""
    assert P8.dtype == np.int64 and int(np.abs(P8).max(initial=0)) < 1 << 20
    if C8 is None:
        return
    for C in C8:
        adj, det = _int_inverse(C)
        assert det & (det - 1) == 0, f"det {det}: the inverse is not dyadic"
        den = det // int(np.gcd.reduce(np.append(np.abs(adj).ravel(), det)))
        assert den <= UNIT << 10
        assert int(np.abs(P8).max(initial=1)) * int(np.abs(adj).max()) < 1 << 40    # the exact arithmetic above stays in int64


def _case(name, P8, rc, C8=None, pbc=None, ptr=None, z=None, note=""):
    P8 = np.ascontiguousarray(P8, dtype=np.int64).reshape(-1, 3)
    ptr = np.array([0, len(P8)], dtype=np.int64) if ptr is None else np.asarray(ptr, dtype=np.int64)
    if C8 is not None:
        C8 = np.asarray(C8, dtype=np.int64).reshape(-1, 3, 3)
        assert len(C8) == len(ptr) - 1
    _assert_dyadic(P8, C8)
    return SimpleNamespace(name=name, P8=P8, C8=C8, pbc=None if pbc is None else [bool(v) for v in pbc], ptr=ptr, rc=float(rc),
                           periodic=C8 is not None, n_atoms=len(P8), z=z, note=note)


def positions(case, dtype):
    return (case.P8.astype(np.float64) / UNIT).astype(dtype)


def cells(case, dtype):
    return (case.C8.astype(np.float64) / UNIT).astype(dtype)


def _sc(nx, ny, nz, step=2 * UNIT):
    """simple cubic grid, x slowest"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.int64) * step


def _diag(a, b, c):
    return np.diag([a * UNIT, b * UNIT, c * UNIT])


RC = 6.0                # every crystal below: 2 A grid, shells at 2, 2.83, 3.46, 4, 4.47, 4.90, 5.66 inside; (6,0,0), (4,4,2) ON the cutoff
RC_GAS = 6.0
RC_OPEN = 5.0           # 1 A grids: (5,0,0), (3,4,0) on the cutoff


@functools.lru_cache(maxsize=None)
def _cases():
    un = np.array(UNWRAP8)
    out = []
    # ---- simple cubic, 2 A grid, rc = 6
    out.append(_case("sc8", _sc(4, 4, 4) + un, RC, _diag(8, 8, 8), [1, 1, 1]))
    out.append(_case("sc16", _sc(8, 8, 8) + un, RC, _diag(16, 16, 16), [1, 1, 1]))
    p = _sc(16, 8, 8)
    p[p[:, 0] == 0, 0] = 32 * UNIT          # the layer at x = 0 is given at x = L: frac == 1 exactly; the rest sits at frac == k/16
    out.append(_case("sc32_faces", p, RC, _diag(32, 16, 16), [1, 1, 1], note="bins (5, 2, 2); atoms at frac == 0 and frac == 1"))
    out.append(_case("sc32_unwrapped", _sc(16, 8, 8) + un, RC, _diag(32, 16, 16), [1, 1, 1], note="bins (5, 2, 2)"))
    # ---- sheared cells (the 2 A grid is invariant under both lattices; the cube [0, 16)^3 holds one atom per lattice class)
    out.append(_case("shear_xy", _sc(8, 8, 8) + un, RC, [[128, 0, 0], [64, 128, 0], [0, 0, 128]], [1, 1, 1]))
    out.append(_case("shear_xy_yz", _sc(8, 8, 8) + un, RC, [[128, 0, 0], [64, 128, 0], [0, 64, 128]], [1, 1, 1]))
    # ---- cells smaller than the cutoff: two images on some axes, every atom its own neighbour, (i, j) repeated with several offsets
    out.append(_case("small444", _sc(2, 2, 2) + un, RC, _diag(4, 4, 4), [1, 1, 1]))
    out.append(_case("small4816", _sc(2, 4, 8) + un, RC, _diag(4, 8, 16), [1, 1, 1]))
    # ---- slab and wire: atoms outside [0, 1) on the open axes stay where they are
    out.append(_case("slab", _sc(8, 8, 4) + un, RC, _diag(16, 16, 16), [1, 1, 0]))
    out.append(_case("wire", _sc(8, 4, 4) + un, RC, _diag(16, 16, 16), [1, 0, 0]))
    # ---- rock salt with every 7th atom taken out: ragged degrees, thin bins
    p = _sc(8, 8, 8)
    z = np.where((p // (2 * UNIT)).sum(1) % 2 == 0, 11, 17)
    keep = np.arange(len(p)) % 7 != 6
    out.append(_case("rocksalt_vacancies", p[keep] + un, RC, _diag(16, 16, 16), [1, 1, 1], z=z[keep]))
    # ---- dyadic gas: random integers on the 1/8 A grid at about the density of water (0.1 atoms / A^3)
    rng = np.random.default_rng(20261018)
    base = rng.integers(0, 16 * UNIT, size=(380, 3))
    dup = np.concatenate([base, base[:30]])                                  # 30 pairs at D == 0
    close = np.concatenate([base, base[:30] + np.array([1, 0, 0])])          # 30 pairs at D == 1/8
    for name, p in (("gas_coincident", dup), ("gas_eighth", close)):
        out.append(_case(name, p + un, RC_GAS, _diag(16, 16, 16), [1, 1, 1]))
        out.append(_case(name + "_open", p + un, RC_GAS))
    # a thin gas in a cell with five bins on EVERY axis (the wrapped b - 1, b, b + 1 walk in three dimensions)
    out.append(_case("gas_bins555", rng.integers(-8 * UNIT, 40 * UNIT, size=(1024, 3)), RC_GAS, _diag(32, 32, 32), [1, 1, 1], note="bins (5, 5, 5)"))
    # ---- several graphs in one call: rep is the maximum over the batch (2, from the 4 A cell), thr and the bins are per graph
    big = _sc(16, 8, 8) + un
    p = np.concatenate([_sc(4, 4, 4) + un, np.array([[5, -3, 70]]), big])
    out.append(_case("batch", p, RC, [_diag(8, 8, 8), _diag(8, 8, 8), _diag(4, 4, 4), _diag(32, 16, 16)], [1, 1, 1],
                     ptr=[0, 64, 64, 65, 65 + len(big)], note="64-atom cube, empty graph, one atom in a 4 A cell, sc32"))
    # ---- open boundary only (1 A grids, rc = 5)
    A = UNIT
    out.append(_case("open_cube", _sc(8, 8, 8, A) + np.array([100 * A, -50 * A, 2]), RC_OPEN))
    out.append(_case("open_sheet", _sc(24, 24, 1, A) + np.array([0, 0, 28]), RC_OPEN))
    out.append(_case("open_line", _sc(200, 1, 1, A // 2) + np.array([-7, 3, 3]), RC_OPEN))
    out.append(_case("open_point", np.tile(np.array([[11, -4, 9]]), (70, 1)), RC_OPEN))
    out.append(_case("open_cube_far", _sc(8, 8, 8, A) + np.array([4096 * A, -4096 * A, 1]), RC_OPEN))
    out.append(_case("open_extent_3rc", _sc(16, 4, 4, A) + np.array([-2 * A, 0, 0]), RC_OPEN,
                     note="extent exactly 3 rc along x: the last atom has (p - lo) inv_w == nb before the clamp"))
    p = np.concatenate([_sc(8, 8, 8, A), np.array([[0, 0, 0]]), _sc(24, 24, 1, A)])
    out.append(_case("open_batch", p, RC_OPEN, ptr=[0, 512, 512, 513, 513 + 576], note="cube, empty graph, lone atom, sheet"))
    return tuple(out)


def all_cases():
    return _cases()


def names(periodic=None):
    return [c.name for c in _cases() if periodic is None or c.periodic == periodic]


def case(name):
    return next(c for c in _cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def exact(name):
    """the exact list of a case, computed once and shared (read-only arrays): (edge_index, cell_offsets or None, ties)"""
    c = case(name)
    if c.periodic:
        out = exact_pbc_list(c.P8, c.C8, c.pbc, c.rc, ptr=c.ptr, count_ties=True)
    else:
        ei, ties = exact_open_list(c.P8, c.ptr, c.rc, count_ties=True)
        out = (ei, None, ties)
    for a in out[:2]:
        if a is not None:
            a.setflags(write=False)
    return out


SINGLE_SYSTEM = ("sc32_faces", "small444", "shear_xy")      # for xeq::radius_graph_pbc (one graph, positions searched as given)


@functools.lru_cache(maxsize=None)
def exact_single_system(name):
    """the list of the single-system form (no wrapping) on the WRAPPED positions of a case: the images -rep .. rep then reach every
    neighbour, and the offsets are the image indices themselves"""
    c = case(name)
    pw, _ = wrap_exact(c.P8, c.C8[0], c.pbc)
    if name == "sc32_faces":
        pw = c.P8                                          # kept as given: atoms at x == L exactly, still every neighbour within one image
    ei, off = exact_pbc_list(pw, c.C8, c.pbc, c.rc, wrap=False)
    return pw, ei, off


# ------------------------------------------------------------------------------------- a shell that sits on the cutoff in rounding
FCC_RC = 5.0
FCC_DISPLACEMENT = 0.05
FCC_VARIANTS = (0, -3)        # a = f32(5 / sqrt 2): f32 drops the whole fourth shell, f64 keeps it; three ulps below: the shell splits (45 edges without a mirror)


def fcc_shell(variant=0, displaced=False):
    """FCC, a = 5 / sqrt(2), 3 x 3 x 3 conventional cells (108 atoms): in real arithmetic the fourth shell (12 atoms) is at 5.0, the
    cutoff, so in f32 its members fall on either side of `<`.  ``variant``: a moved by that many f32 ulps.  ``displaced``: every atom
    moved by a fixed pseudo-random vector of length 0.05 A (no tie left, finite forces).  -> pos [108, 3] f32, z, ptr, cell [1, 3, 3]
    f32: the f32 numbers ARE the input; the f64 evaluations take them exactly."""
    a = np.float32(5.0 / np.sqrt(2.0))
    for _ in range(abs(variant)):
        a = np.nextafter(a, np.float32(np.inf if variant > 0 else -np.inf), dtype=np.float32)
    a = float(a)
    basis = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    corner = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    pos = ((corner + basis[None]).reshape(-1, 3) * a)
    if displaced:
        v = np.random.default_rng(108).normal(size=pos.shape)
        pos = pos + FCC_DISPLACEMENT * v / np.linalg.norm(v, axis=1, keepdims=True)
    cell = (np.eye(3) * 3 * a)[None]
    return pos.astype(np.float32), np.full(len(pos), 8, dtype=np.int32), np.array([0, len(pos)], dtype=np.int64), cell.astype(np.float32)


def list_differences(ei_a, off_a, ei_b, off_b):
    """number of (i, j, o) held by exactly one of two lists"""
    def rows(ei, off):
        return {tuple(r) for r in np.concatenate([ei.T, np.asarray(off).astype(np.int64)], axis=1).tolist()}
    return len(rows(ei_a, off_a) ^ rows(ei_b, off_b))


# ------------------------------------------------------------------------------------------------------------------- bin edges
# Not dyadic: atoms ON a bin edge and one f32 step to either side of it, each with partners along the same axis 2^-12 rc inside and
# outside the cutoff -- four orders above f32 rounding, so the f64 list of the same f32 numbers is unambiguous (``distance_margins``)
# and nothing is excluded.
EDGE_EPS = 2.0 ** -12


def _hairs(x):
    x = np.float32(x)
    return [x, np.nextafter(x, np.float32(-np.inf), dtype=np.float32), np.nextafter(x, np.float32(np.inf), dtype=np.float32)]


def _with_partners(xs, rc, lo=-np.inf, hi=np.inf):
    out = []
    for x in xs:
        out.append(np.float32(x))
        for sign in (1.0, -1.0):
            for e in (-EDGE_EPS, EDGE_EPS):
                p = np.float32(float(x) + sign * rc * (1.0 + e))
                if lo < p < hi:
                    out.append(p)
    return out


def _axis_graphs(per_axis, rest=(3.0, 5.0)):
    """one graph per axis: the coordinates of per_axis[ax] along ax, the other two fixed -> pos f32 [n, 3], ptr"""
    pos, ptr = [], [0]
    for ax in range(3):
        p = np.empty((len(per_axis[ax]), 3), dtype=np.float32)
        p[:, ax] = per_axis[ax]
        p[:, (ax + 1) % 3], p[:, (ax + 2) % 3] = rest
        pos.append(p)
        ptr.append(ptr[-1] + len(p))
    return np.concatenate(pos), np.array(ptr, dtype=np.int64)


def bin_edge_case_pbc(cell, nb, rc):
    """cell [3, 3] diagonal (f32), nb [3] the bins the code computes: atoms at frac = k / nb and a step to either side (and, a hair
    below 0, at -2^-26 L: in f32 its wrapped fractional coordinate 1 - 2^-26 rounds to 1.0, the far face), partners at +-rc (1 +- 2^-12)."""
    per_axis = []
    for ax in range(3):
        L = float(cell[ax, ax])
        xs = [h for k in range(int(nb[ax])) for h in _hairs(L * k / int(nb[ax]))] + [np.float32(-L * 2.0 ** -26)]
        per_axis.append(_with_partners(xs, rc))
    return _axis_graphs(per_axis)


OPEN_EDGE_ANCHORS = (-10.0, 31.0)      # two corner atoms fix the bounding box: extent 41 = 8 bins of 5.125 at rc = 5


def bin_edge_case_open(lo, nb, inv_w, rc):
    """lo, nb, inv_w [3] as ops._box_grid computes them for the anchors: atoms at lo + k * width (0 < k < nb) and a step to either
    side, partners at +-rc (1 +- 2^-12) where they stay inside the box (the box must not move)."""
    per_axis = []
    for ax in range(3):
        a, b = OPEN_EDGE_ANCHORS
        xs = [h for k in range(1, int(nb[ax])) for h in _hairs(np.float32(lo[ax]) + np.float32(k) / np.float32(inv_w[ax]))]
        per_axis.append(_with_partners(xs, rc, a, b))
    pos, ptr = _axis_graphs(per_axis)
    anchors = np.array([[OPEN_EDGE_ANCHORS[0]] * 3, [OPEN_EDGE_ANCHORS[1]] * 3], dtype=np.float32)
    out, new_ptr = [], [0]
    for g in range(3):
        out += [anchors[:1], pos[ptr[g]:ptr[g + 1]], anchors[1:]]
        new_ptr.append(new_ptr[-1] + ptr[g + 1] - ptr[g] + 2)
    return np.concatenate(out), np.array(new_ptr, dtype=np.int64)


def distance_margins(pos, ptr, rc, cell=None, pbc=None):
    """(min |D - rc|, min |D - 0.01|) over all pairs (and images) in f64 on the given numbers"""
    pos = np.asarray(pos, dtype=np.float64)
    m_rc = m_lo = np.inf
    for g in range(len(ptr) - 1):
        p = pos[ptr[g]:ptr[g + 1]]
        if cell is None:
            img = np.zeros((1, 3))
        else:
            c = np.asarray(cell[g], dtype=np.float64)
            reps = orc._n_images(c[None], pbc, rc)
            img = _grid([r + 1 if pbc[ax] else 0 for ax, r in enumerate(reps)]).astype(np.float64) @ c      # one image more: wrapping moves atoms
        d = p[:, None, None, :] - p[None, :, None, :] - img[None, None, :, :]
        D = np.sqrt((d * d).sum(-1))
        m_rc, m_lo = min(m_rc, float(np.abs(D - rc).min())), min(m_lo, float(np.abs(D - 0.01).min()))
    return m_rc, m_lo
